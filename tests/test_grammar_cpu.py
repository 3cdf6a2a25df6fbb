"""Regex-constrained generation, CPU branch: ``grammar.compile_regex`` against Python's ``re`` on every string of a small alphabet, the
shape of the automata (trimmed, within the limits, minimal), what the compiler refuses, ``grammar.token_byte_table``, the host form of
``fused_ops.grammar_mask`` against the oracle (tests/_grammar_oracle.py) bit for bit, the declarations, and ``ChatGLMDecoder.generate_ids``
/ ``generate_batch_ids`` with ``grammar=`` on the CPU tiny model over a synthetic vocabulary.  The GPU twin (the HIP kernel, the captured
"+gr" steps) is test_grammar_gpu.py."""
import itertools
import os
import random
import re

import numpy as np
import pytest
import torch

import _grammar_oracle as GO
from chatglm_q_amd import _lib, fused_ops
from chatglm_q_amd import grammar as G
from chatglm_q_amd.decoder import ChatGLMDecoder
from test_model_cpu import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}

# every supported construct; the alphabet below holds a three-byte character that is neither \w nor \s nor \d, a newline and a space
PATTERNS = [
    "a", "ab|b", "a*", "(a|b)+", "a?b", "a{2}", "a{1,3}b", "a{2,}", "a{,2}", "[ab]", "[^a]", "[^ab]+", ".", ".*a", "(a(b|€)){1,2}", "(?:ab)*€?",
    "\\d+", "[a\\d]{1,2}", "\\w\\s?", "^ab$", "a|", "€+", "[€a]b", "1\\.", "(a|b|1)(a|b|1)?", "\\D", "\\S\\W", "a\\nb|.", "((a|b){2}){1,2}",
    "[a-b1]*\\n?", "(a|(b|(1|€)))\\x20?", "\\$?a\\|", "[]a]|[b-]",
]
ALPHABET = ["a", "b", "1", "€", "\n", " "]


def to_bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32).numpy().view(np.uint16 if t.element_size() == 2 else np.uint32).copy()


# ---- the compiler ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", PATTERNS)
def test_compiler_equals_re(pattern):
    dfa = G.compile_regex(pattern)
    alphabet = ALPHABET + (["$", "|", "]", "-"] if pattern in ("\\$?a\\|", "[]a]|[b-]") else [])
    top = 6 if len(alphabet) <= 6 else 4
    for L in range(top + 1):
        for chars in itertools.product(alphabet[:5] if L == 6 else alphabet, repeat=L):
            s = "".join(chars)
            assert dfa.matches(s.encode()) == bool(re.fullmatch(pattern, s)), (pattern, s)


@pytest.mark.parametrize("pattern", PATTERNS + ["-?[0-9]{1,3}", "(yes|no)", "[A-D]", '\\{("[a-z]+":("[^"]*"|-?[0-9]+)(,"[a-z]+":("[^"]*"|-?[0-9]+))*)?\\}'])
def test_shape_of_the_automaton(pattern):
    dfa = G.compile_regex(pattern)
    assert dfa.table.shape == (dfa.n_states, dfa.n_classes) and dfa.table.dtype == np.uint16
    assert dfa.class_of.shape == (256,) and dfa.class_of.dtype == np.uint8 and int(dfa.class_of.max()) == dfa.n_classes - 1
    assert dfa.accept.shape == (dfa.n_states,) and dfa.accept.any()
    assert dfa.n_states <= G.GRAMMAR_STATES_MAX and dfa.n_states * dfa.n_classes <= G.GRAMMAR_TABLE_MAX
    live = dfa.table[dfa.table != G.DEAD]
    assert live.size == 0 or int(live.max()) < dfa.n_states
    # trimmed: every state reaches an accepting one (so a live state can always finish), and the start reaches every state
    reach = set(np.nonzero(dfa.accept)[0].tolist())
    changed = True
    while changed:
        changed = False
        for s in range(dfa.n_states):
            if s not in reach and any(t != G.DEAD and int(t) in reach for t in dfa.table[s]):
                reach.add(s)
                changed = True
    assert reach == set(range(dfa.n_states))
    seen, stack = {0}, [0]
    while stack:
        for t in dfa.table[stack.pop()]:
            if t != G.DEAD and int(t) not in seen:
                seen.add(int(t))
                stack.append(int(t))
    assert seen == set(range(dfa.n_states))
    # byte classes: no two columns are equal; minimal: no two states have the same row and flag, and minimising again changes nothing
    assert len({tuple(col) for col in dfa.table.T.tolist()}) == dfa.n_classes
    assert len({(tuple(row), int(a)) for row, a in zip(dfa.table.tolist(), dfa.accept)}) == dfa.n_states
    again = G.minimize(dfa)
    assert again.n_states == dfa.n_states and np.array_equal(again.table, dfa.table) and np.array_equal(again.class_of, dfa.class_of)
    assert np.array_equal(again.accept, dfa.accept)


def test_minimisation_merges_equivalent_states():
    assert G.compile_regex("(ab|cb)").n_states == G.compile_regex("[ac]b").n_states == 3
    assert G.compile_regex("a|a|a").n_states == 2 and G.compile_regex("(a*)*").n_states == 1
    d = G.compile_regex("x{100}")
    assert (d.n_states, d.n_classes) == (101, 2)
    assert np.array_equal(G.compile_regex("a{2,3}").table, G.compile_regex("aaa?").table)


def test_step_matches_and_choices():
    d = G.compile_regex("-?[0-9]{1,3}")
    assert d.start == 0 and d.step(0, b"") == 0 and d.step(0, b"-1") >= 0 and d.step(0, b"--") == -1 and d.step(-1, b"1") == -1
    assert d.step(d.step(0, b"-"), b"12") == d.step(0, b"-12") and d.accepting(d.step(0, b"-12")) and not d.accepting(d.step(0, b"-"))
    assert d.matches(b"007") and not d.matches(b"1234") and not d.matches(b"")
    c = G.ByteDFA.from_choices(["A", "B", "C.", "好"])
    assert [c.matches(s.encode()) for s in ("A", "B", "C.", "Cx", "好", "AB", "")] == [True, True, True, False, True, False, False]
    assert G.as_dfa(c) is c and G.as_dfa("[A-D]").matches(b"D")
    with pytest.raises(ValueError):
        G.as_dfa(7)
    with pytest.raises(ValueError):
        G.ByteDFA.from_choices([])
    # "." and a negated class take whole UTF-8 characters only: the output always decodes
    dot = G.compile_regex(".*")
    for good in ("é€好𝄞", "a߿b", "퟿"):
        assert dot.matches(good.encode())
    for bad in (b"\x80", b"\xc3", b"\xc0\x80", b"\xe0\x80\x80", b"\xed\xa0\x80", b"\xf4\x90\x80\x80", b"\xf8\x88\x80\x80\x80", b"a\n"):
        assert not dot.matches(bad), bad


@pytest.mark.parametrize("pattern,names", [
    ("(a)\\1", "backreference"), ("(?=a)b", "lookaround"), ("(?!a)b", "lookaround"), ("(?<=a)b", "lookaround"), ("(?<!a)b", "lookaround"),
    ("a*?", "lazy"), ("a+?", "lazy"), ("a??", "lazy"), ("a{1,2}?", "lazy"), ("a*+", "possessive"), ("a++", "possessive"),
    ("(?i)a", "flag"), ("(?s:a)", "flag"), ("[α-ω]", "non-ASCII range"), ("[a-ω]", "non-ASCII range"), ("[^é]", "non-ASCII"),
    ("(?P<n>a)", "named group"), ("a^b", "anchor"), ("a$b", "anchor"), ("\\bx", "\\b"), ("\\Ax", "\\A"), ("[[:alpha:]]", "POSIX"),
])
def test_unsupported_constructs_are_named(pattern, names):
    with pytest.raises(ValueError, match=re.escape(names)):
        G.compile_regex(pattern)


@pytest.mark.parametrize("pattern", ["(a", "a)", "[a", "*a", "a{3,1}", "a{x}", "a\\", "a{5000}", "[b-a]", "\\xzz", 7])
def test_malformed_patterns_raise(pattern):
    with pytest.raises(ValueError):
        G.compile_regex(pattern)


def test_a_pattern_over_the_limits_raises_with_both_numbers():
    with pytest.raises(ValueError, match=r"4096 states x 2 byte classes = 8192 table entries \(at most 16384 entries.*4095 states"):
        G.compile_regex("a{4095}")                              # too many states for a table that would fit
    assert G.compile_regex("a{4094}").n_states == 4095
    with pytest.raises(ValueError, match=r"3201 states x 17 byte classes = 54417 table entries \(at most 16384 entries.*4095 states"):
        G.compile_regex("(abcdefghijklmnop){200}")             # states that would fit, a table that does not
    with pytest.raises(ValueError):
        G.ByteDFA(np.zeros(256, np.uint8), np.zeros((4096, 1), np.uint16), np.ones(4096, np.uint8))
    with pytest.raises(ValueError, match="NFA states"):
        G.compile_regex("((a{1000}){1000}){10}")                # refused before anything is unrolled that far


# ---- the vocabulary's byte table --------------------------------------------------------------------------------------------------------
def test_token_byte_table_from_a_byte_list_round_trips():
    toks = GO.make_vocab(300, seed=4, singles=b"abc")
    tb = G.token_byte_table(toks)
    assert len(tb) == 300 and tb.off.dtype == np.int32 and tb.bytes.dtype == np.uint8 and tb.off.shape == (301,)
    assert tb.tokens() == toks and [tb.token(i) for i in (0, 17, 299)] == [toks[0], toks[17], toks[299]]
    assert tb.off[0] == 0 and tb.off[-1] == tb.bytes.size == sum(len(t) for t in toks) and b"" in toks and max(len(t) for t in toks) == 40
    assert tb.join([3, 299, 5, -1, 300]) == toks[3] + toks[299] + toks[5]         # ids outside the table count as empty
    assert G.token_byte_table(tb) is tb
    wide = tb.padded(320)
    assert len(wide) == 320 and wide.tokens()[:300] == toks and wide.tokens()[300:] == [b""] * 20 and tb.padded(300) is tb
    with pytest.raises(ValueError):
        tb.padded(299)
    with pytest.raises(ValueError):
        G.token_byte_table(["text"])
    with pytest.raises(ValueError):
        G.token_byte_table(object())


def test_token_byte_table_from_a_sentencepiece_model(tmp_path):
    sentencepiece = pytest.importorskip("sentencepiece")
    from chatglm_q_amd.decoder import SentencePieceIds
    corpus = tmp_path / "corpus.txt"
    corpus.write_text("\n".join([f"the quick brown fox jumps over the lazy dog {i}" for i in range(200)] +
                                ["hello world this is a tiny corpus for a tiny model"] * 50))
    sentencepiece.SentencePieceTrainer.train(input=str(corpus), model_prefix=str(tmp_path / "sentencepiece"), vocab_size=330, model_type="bpe",
                                             normalization_rule_name="identity", byte_fallback=True, minloglevel=2)
    tok = SentencePieceIds(tmp_path / "sentencepiece.model")
    sp = tok.sp
    tb = G.token_byte_table(tok)
    assert len(tb) == len(tok) == len(sp) + 5
    for name in ("<unk>", "<s>", "</s>"):
        assert tb.token(sp.piece_to_id(name)) == b""            # unknown and control pieces
    assert tb.tokens()[len(sp):] == [b""] * 5                   # the five special tokens behind the sentencepiece vocabulary
    assert tb.token(sp.piece_to_id("<0x41>")) == b"A" and tb.token(sp.piece_to_id("<0xE2>")) == b"\xe2"
    assert tb.token(sp.piece_to_id("▁the")) == b" the"
    for text in ("hello world", "the lazy dog 17", "héllo €uro 好 ZZZ", "a", "tiny model jumps"):
        ids = sp.encode(text)
        assert tb.join(ids) == (" " + text).encode(), text      # sentencepiece's own decode drops that one leading space
        assert sp.decode(ids) == text
        assert tb.join(tok.encode(text)) == (" " + text).encode()    # [gMASK] <sop> in front: empty

    class Ref:                                                   # the reference's tokenizer object names its file as vocab_file
        vocab_file = str(tmp_path / "sentencepiece.model")
    assert G.token_byte_table(Ref()).tokens() == tb.tokens()


# ---- the host form against the oracle -------------------------------------------------------------------------------------------------------
HOST_PATTERNS = ["(yes|no)", "[A-D]", "-?[0-9]{1,3}", "[a-d]*", "a.c", "[^a]+,", "(ab|cd)*e?"]


@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
def test_host_form_equals_oracle(dt):
    rng = random.Random({"f16": 16, "bf16": 61, "f32": 32}[dt])
    g = torch.Generator().manual_seed(7)
    dfas = [G.compile_regex(p) for p in HOST_PATTERNS]
    for case in range(24):
        B, N = rng.choice([1, 3, 4]), rng.choice([1, 7, 40, 130])
        n_vocab = rng.choice([N, N, max(1, N - 3), N + 5])
        vocab = GO.make_vocab(n_vocab, seed=case, singles=b"yesnoABCD-0123456789abcde,")
        st = fused_ops.GrammarState(B, G.token_byte_table(vocab), "cpu")
        rows = [dict(dfa=rng.choice(dfas + [None]), state=0, eos=rng.choice([-1, rng.randrange(N)]), N=N) for _ in range(B)]
        st.arm([r["dfa"] for r in rows], [r["eos"] for r in rows])
        with_rows = case % 2 == 0
        row_state = [[0, GO.FINISHED if rng.random() < 0.2 else 0] for _ in rows] if with_rows else None
        rs_t = torch.tensor(row_state, dtype=torch.int32) if with_rows else None
        for step in range(4):
            x = (torch.randn(B, N, generator=g) * 3).to(DT[dt])
            bits = to_bits(x)
            tok = None if step == 0 else [rng.choice([rng.randrange(N), rng.randrange(N), -1, N, N + 7, 2 ** 40]) for _ in range(B)]
            if step == 3:                                       # ... and a dead state on some rows
                for b, r in enumerate(rows):
                    if r["dfa"] is not None and rng.random() < 0.4:
                        r["state"] = -1
                        st.state[b] = -1
            GO.launch(bits, dt, rows, vocab, tok, row_state)
            out = fused_ops.grammar_mask(x, st, None if tok is None else torch.tensor(tok, dtype=torch.int64), rs_t)
            assert out is x
            assert np.array_equal(to_bits(x), bits), (dt, case, step)
            assert st.states() == [r["state"] if r["dfa"] is not None else 0 for r in rows], (dt, case, step)
            assert st.ticket.tolist() == [0] * B


def test_host_form_cases():
    vocab = [b"A", b"B", b"", b"AB", b"x", b""]                  # id 2 is empty, id 5 is the end id (empty as well)
    d = G.compile_regex("AB?")
    st = fused_ops.GrammarState(2, G.token_byte_table(vocab), "cpu").arm([d, None], [5, 5])
    x = torch.zeros(2, 6)
    fused_ops.grammar_mask(x, st)
    assert torch.isinf(x[0]).tolist() == [False, True, True, False, True, True] and not torch.isinf(x[1]).any()      # start: "A" or "AB"
    x.zero_()
    fused_ops.grammar_mask(x, st, torch.tensor([0, 0]))          # fed "A": accepting, "B" may follow
    assert torch.isinf(x[0]).tolist() == [True, False, True, True, True, False] and st.states()[0] == d.step(0, b"A")
    x.zero_()
    fused_ops.grammar_mask(x, st, torch.tensor([1, 0]))          # fed "B": accepting with no continuation - only the end id survives
    assert torch.isinf(x[0]).tolist() == [True, True, True, True, True, False]
    keep = st.states()
    x.zero_()
    fused_ops.grammar_mask(x, st, torch.tensor([5, 0]))          # fed the end id (empty): nothing moves
    assert st.states() == keep and torch.isinf(x[0]).tolist() == [True, True, True, True, True, False]
    x.zero_()
    fused_ops.grammar_mask(x, st, torch.tensor([4, 0]))          # fed "x": dead - everything but the end id is masked, the row ends
    assert st.states()[0] == -1 and torch.isinf(x[0]).tolist() == [True, True, True, True, True, False] and not torch.isinf(x[1]).any()


def test_argument_errors():
    vocab = G.token_byte_table([b"a", b"b", b"c"])
    d = G.compile_regex("a")
    with pytest.raises(ValueError):
        fused_ops.GrammarState(0, vocab, "cpu")
    with pytest.raises(ValueError):
        fused_ops.GrammarState(1, [b"a"], "cpu")
    st = fused_ops.GrammarState(2, vocab, "cpu")
    for bad in (([d], None), ([d, "a"], None), ([d, d], [0]), ([d, d], [0, -2]), ([d, d], [0, "x"])):
        with pytest.raises(ValueError):
            st.arm(*bad)
    st.arm([d, None], [2, None])
    assert st.cfg.tolist() == [[2, 2], [0, -1]] and st.active and st.states() == [0, 0]
    assert not fused_ops.GrammarState(2, vocab, "cpu").arm(None).active
    with pytest.raises(ValueError):
        fused_ops.grammar_mask(torch.zeros(3), st)
    with pytest.raises(ValueError):
        fused_ops.grammar_mask(torch.zeros(1, 3), st)
    with pytest.raises(ValueError):
        fused_ops.grammar_mask(torch.zeros(2, 6)[:, ::2], st)
    with pytest.raises(ValueError):
        fused_ops.grammar_mask(torch.zeros(1, 3).expand(2, 3), st)
    with pytest.raises(ValueError):
        fused_ops.grammar_mask(torch.zeros(2, 3), st, torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError):
        fused_ops.grammar_mask(torch.zeros(2, 3), st, row_state=torch.zeros(2, 2))
    with pytest.raises(ValueError):
        fused_ops.grammar_mask(torch.zeros(2, 3), object())


def test_declarations():
    header = open(os.path.join(ROOT, "include", "qlinear_hip.h")).read()
    assert re.search(r"^int qlinear_grammar_mask\(", header, re.M)
    assert re.search(r"^#define QLINEAR_ABI_VERSION 3$", header, re.M) and "Still 3: qlinear_grammar_mask" in header
    for name, value in (("TABLE_MAX", fused_ops.GRAMMAR_TABLE_MAX), ("STATES_MAX", fused_ops.GRAMMAR_STATES_MAX), ("CHUNK", fused_ops.GRAMMAR_CHUNK)):
        assert re.search(rf"^#define QL_GRAMMAR_{name} {value}$", header, re.M)
    assert (fused_ops.GRAMMAR_TABLE_MAX, fused_ops.GRAMMAR_STATES_MAX) == (G.GRAMMAR_TABLE_MAX, G.GRAMMAR_STATES_MAX) == (16384, 4095)
    assert "qlinear_grammar_mask" in _lib.EXPORTS
    makefile = open(os.path.join(ROOT, "chatglm_q_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", makefile, re.M).group(1).split()
    assert "grammar_mask.hip" in srcs and os.path.exists(os.path.join(ROOT, "chatglm_q_amd", "csrc", "grammar_mask.hip"))


# ---- the tiny model ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_f32():
    return build("f32")


PROMPT = [17, 3, 99, 250, 8, 61]
PROMPTS = [[5, 9, 200, 31, 7, 44, 3, 12], [44, 3], [100, 101, 102, 0], [250]]
LANGUAGES = {"(yes|no)": 3, "[A-D]": 1, "-?[0-9]{1,3}": 4}       # a finite language and its longest word, in bytes
WORDS = (b"yes", b"no", b"ye", b"es", b"12", b"-1", b"007", b"AB", b"noo", b"-")


def tiny_vocab(n):
    """A vocabulary for the tiny model: the languages' single bytes and some of their multi-byte pieces among random tokens; the end id
    is the id of an empty token."""
    vocab = GO.make_vocab(n, seed=11, singles=b"yesnoABCD-0123456789", extra=WORDS)
    eos = [i for i, t in enumerate(vocab) if not t][1]
    assert eos not in PROMPT and all(eos not in q for q in PROMPTS)          # (so no prompt feeds it to the model)
    return vocab, eos


def check_row(dfa_pattern, ids, eos, vocab, state):
    assert ids and ids[-1] == eos and eos not in ids[:-1], (dfa_pattern, ids)
    text = b"".join(vocab[i] for i in ids[:-1])
    assert re.fullmatch(dfa_pattern.encode(), text), (dfa_pattern, text)
    assert all(len(vocab[i]) > 0 for i in ids[:-1]) and state == "accepted"


@pytest.mark.parametrize("pattern", sorted(LANGUAGES))
def test_generate_ids_matches_the_pattern(pattern, tiny_f32):
    model, cfg = tiny_f32
    vocab, eos = tiny_vocab(cfg.vocab_size)
    dec = ChatGLMDecoder(cfg, model, eos_token_id=eos, token_bytes=vocab)
    budget = LANGUAGES[pattern] + 1                              # every token holds a byte at least: the longest word and the end token fit
    base = list(dec.generate_ids(PROMPT, max_generated_tokens=budget, greedy=True))
    assert dec.last_stats["grammar"] is False and dec.last_stats["grammar_state"] is None and dec._session.gr is None
    for mode in (dict(greedy=True), dict(seed=5), dict(seed=6, top_k=3), dict(seed=7, device_sampler=False)):
        for g in (pattern, G.compile_regex(pattern)):
            ids = list(dec.generate_ids(PROMPT, max_generated_tokens=budget, grammar=g, **mode))
            check_row(pattern, ids, eos, vocab, dec.last_stats["grammar_state"])
            assert dec.last_stats["grammar"] is True
    assert list(dec.generate_ids(PROMPT, max_generated_tokens=budget, greedy=True)) == base         # ... and off again
    # a budget that ends inside the pattern: "open"
    ids = list(dec.generate_ids(PROMPT, max_generated_tokens=1, greedy=True, grammar=pattern))
    assert len(ids) == 1 and ids[0] != eos and dec.last_stats["grammar_state"] == "open"
    assert G.compile_regex(pattern).step(0, vocab[ids[0]]) >= 0


def test_generate_batch_ids_per_prompt(tiny_f32):
    model, cfg = tiny_f32
    vocab, eos = tiny_vocab(cfg.vocab_size)
    dec = ChatGLMDecoder(cfg, model, eos_token_id=eos, token_bytes=G.token_byte_table(vocab))
    pats = ["(yes|no)", None, "-?[0-9]{1,3}", G.compile_regex("[A-D]")]
    for mode in (dict(greedy=True), dict(seed=[3, 4, 5, 6])):
        plain = dec.generate_batch_ids(PROMPTS, max_generated_tokens=5, **mode)
        assert dec.last_stats["grammar"] is False and dec.last_stats["grammar_state"] == [None] * 4
        got = dec.generate_batch_ids(PROMPTS, max_generated_tokens=5, grammar=pats, **mode)
        states = dec.last_stats["grammar_state"]
        assert dec.last_stats["grammar"] is True and states[1] is None
        assert got[1] == plain[1]                                # the row without a grammar: the ids of the same call without
        for b, p in ((0, "(yes|no)"), (2, "-?[0-9]{1,3}"), (3, "[A-D]")):
            check_row(p, got[b], eos, vocab, states[b])
    # one pattern for every row; a batch of one equals generate_ids
    got = dec.generate_batch_ids(PROMPTS, max_generated_tokens=2, greedy=True, grammar="[A-D]")
    for b in range(4):
        check_row("[A-D]", got[b], eos, vocab, dec.last_stats["grammar_state"][b])
    one = dec.generate_batch_ids([PROMPT], max_generated_tokens=5, greedy=True, grammar="-?[0-9]{1,3}")
    assert one == [list(dec.generate_ids(PROMPT, max_generated_tokens=5, greedy=True, grammar="-?[0-9]{1,3}"))]


def test_api_argument_errors(tiny_f32):
    model, cfg = tiny_f32
    vocab, eos = tiny_vocab(cfg.vocab_size)
    dec = ChatGLMDecoder(cfg, model, eos_token_id=eos, token_bytes=vocab)
    with pytest.raises(ValueError, match="end token"):
        list(dec.generate_ids(PROMPT, max_generated_tokens=3, greedy=True, grammar="[A-D]", ignore_eos=True))
    with pytest.raises(ValueError, match="end token"):
        list(ChatGLMDecoder(cfg, model, token_bytes=vocab).generate_ids(PROMPT, max_generated_tokens=3, greedy=True, grammar="[A-D]"))
    with pytest.raises(ValueError, match="min_new_tokens"):
        list(dec.generate_ids(PROMPT, max_generated_tokens=3, greedy=True, grammar="[A-D]", min_new_tokens=2))
    with pytest.raises(ValueError, match="min_new_tokens"):
        dec.generate_batch_ids(PROMPTS, max_generated_tokens=3, greedy=True, grammar=[None, "[A-D]", None, None], min_new_tokens=[0, 2, 0, 0])
    dec.generate_batch_ids(PROMPTS, max_generated_tokens=3, greedy=True, grammar=[None, "[A-D]", None, None], min_new_tokens=[2, 0, 2, 2])
    with pytest.raises(ValueError, match="byte table"):
        list(ChatGLMDecoder(cfg, model, eos_token_id=eos).generate_ids(PROMPT, max_generated_tokens=3, greedy=True, grammar="[A-D]"))
    with pytest.raises(ValueError):
        list(dec.generate_ids(PROMPT, max_generated_tokens=3, greedy=True, grammar="(a"))
    with pytest.raises(ValueError):
        dec.generate_batch_ids(PROMPTS, max_generated_tokens=3, grammar=["a", "b"])
    with pytest.raises(TypeError):
        dec.beam_search_ids(PROMPT, num_beams=2, max_generated_tokens=3, grammar="[A-D]")

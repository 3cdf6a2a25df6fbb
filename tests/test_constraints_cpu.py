"""History constraints, CPU branch: the oracle (tests/_constraints_oracle.py) against hand-written cases, the host form of
``fused_ops.history_constraints`` against the oracle, ``ConstraintState``'s validation, the declarations, and
``ChatGLMDecoder.generate_ids`` / ``generate_batch_ids`` with no_repeat_ngram_size / bad_words_ids / stop_sequences / min_new_tokens on
the CPU tiny model, each test asserting its own precondition.  The GPU twin (the HIP kernel, the captured "+con" steps) is
test_constraints_gpu.py."""
import os
import random
import re

import numpy as np
import pytest
import torch

import _constraints_oracle as CO
from chatglm_q_amd import _lib, fused_ops
from chatglm_q_amd.decoder import ChatGLMDecoder
from test_model_cpu import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAN, STOP, MIN = CO.BAN, CO.STOP, CO.MIN


# ---- the oracle against literal expectations ----------------------------------------------------------------------------------------
def test_oracle_ngram_rule():
    assert CO.ngram_bans([1, 2, 3, 1, 2], 3) == {3}
    assert CO.ngram_bans([1, 2, 3, 1, 2], 1) == {1, 2, 3}
    assert CO.ngram_bans([5, 5], 2) == {5}
    assert CO.ngram_bans([1, 2], 3) == set()                     # L = n - 1: the range of i is empty
    assert CO.ngram_bans([1], 3) == set() and CO.ngram_bans([], 3) == set() and CO.ngram_bans([], 1) == set()   # L < n - 1
    assert CO.ngram_bans([1, 2, 3, 1, 2], 0) == set()
    assert CO.ngram_bans([7, 8, 9, 7, 8, 4, 7, 8], 3) == {9, 4}
    assert CO.ngram_bans([7, 8, 9, 7, 8], 2) == {9}             # the last id is 8: what followed an 8


def test_oracle_sequences_and_min():
    assert CO.sequence_bans([4, 1, 2], 0, [(BAN, [1, 2, 9])], 0) == {9}
    assert CO.sequence_bans([4, 2, 1], 0, [(BAN, [1, 2, 9])], 0) == set()
    assert CO.sequence_bans([4, 1, 2], 3, [(BAN, [1, 2, 9])], 0) == {9}          # the prompt counts
    assert CO.sequence_bans([2], 0, [(BAN, [1, 2, 9])], 0) == set()              # shorter than the head
    assert CO.sequence_bans([], 0, [(BAN, [6])], 0) == {6} and CO.sequence_bans([1, 2, 3], 1, [(BAN, [6])], 0) == {6}
    # MIN: P = 2, min_new = 3: g = 2 bans, g = 3 does not
    assert CO.sequence_bans([1, 2, 3, 4], 2, [(MIN, [8])], 3) == {8}
    assert CO.sequence_bans([1, 2, 3, 4, 5], 2, [(MIN, [8])], 3) == set()
    assert CO.sequence_bans([1, 2], 2, [(MIN, [8])], 0) == set()
    assert CO.sequence_bans([4, 1, 2], 0, [(STOP, [1, 2, 9])], 0) == set()       # a STOP entry bans nothing


def test_oracle_stop():
    table = [(BAN, [3, 4]), (STOP, [9, 9, 9]), (STOP, [3, 4]), (STOP, [4])]
    assert CO.stop_index([1, 2, 3, 4], 2, table) == 2            # inside the generated ids; the smallest index wins (3 matches too)
    assert CO.stop_index([1, 2, 3, 4], 3, table) == 3            # [3, 4] straddles the prompt boundary: no match; [4] is generated
    assert CO.stop_index([1, 2, 3, 4], 4, table) is None         # nothing generated
    assert CO.stop_index([1, 2, 3, 4, 5], 2, table) is None      # not at the end
    assert CO.stop_index([3, 4], 0, [(BAN, [3, 4])]) is None


def test_oracle_launch_order_of_the_rules():
    # append first, then stop (logits untouched, live drops), otherwise bans; a finished row: nothing at all
    rows = [dict(hist=[1, 2], P=1, n=2, min_new=0, table=[(STOP, [2, 3])], N=8),
            dict(hist=[1, 2], P=1, n=2, min_new=0, table=[(STOP, [2, 3])], N=8),
            dict(hist=[1, 2, 3, 2], P=1, n=2, min_new=0, table=[], N=8)]
    bits = np.zeros((3, 8), dtype=np.uint16)
    row_state = [[1, 0], [1, CO.FINISHED], [3, 0]]
    live = CO.launch(bits, "f16", rows, 5, tok=[3, 3, 3], row_state=row_state, live=2)
    assert live == 1 and row_state == [[1, CO.FINISHED], [1, CO.FINISHED], [3, 0]]
    assert rows[0]["hist"] == [1, 2, 3] and rows[1]["hist"] == [1, 2] and rows[2]["hist"] == [1, 2, 3, 2, 3]
    assert not bits[:2].any() and np.flatnonzero(bits[2]).tolist() == [2] and bits[2, 2] == 0xFC00
    CO.launch(bits, "f16", rows, 5, tok=[3, 3, 3])               # row 2 is full: nothing is appended, the bans go on
    assert rows[2]["hist"] == [1, 2, 3, 2, 3] and rows[0]["hist"] == [1, 2, 3, 3]


# ---- the host form against the oracle -------------------------------------------------------------------------------------------------
DT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}


def to_bits(x: torch.Tensor) -> np.ndarray:
    return x.contiguous().view(torch.int16 if x.element_size() == 2 else torch.int32).numpy().view(CO.BITS["f16" if x.element_size() == 2 else "f32"]).copy()


def random_case(rng, B, N, hist_ld, alphabet=5, max_seqs=6):
    """Rows over a small alphabet (matches are frequent) with a few ids of the whole vocabulary."""
    rows, prompts, settings = [], [], []
    for b in range(B):
        L = rng.randrange(0, hist_ld)
        P = rng.randrange(0, L + 1)
        ids = [rng.randrange(min(alphabet, N)) if rng.random() < 0.9 else rng.randrange(N) for _ in range(L)]
        table = []
        for _ in range(rng.randrange(0, max_seqs + 1)):
            kind = rng.choice([BAN, BAN, STOP])
            table.append((kind, [rng.randrange(min(alphabet, N)) for _ in range(rng.choice([1, 1, 2, 2, 3, 5]))]))
        min_new = rng.choice([0, 0, 3, 40])
        if min_new:
            table.append((MIN, [rng.randrange(N)]))
        table.sort(key=lambda e: e[0])                           # ConstraintState.check's order: BAN, STOP, MIN
        n = rng.choice([0, 1, 2, 2, 3, 4])
        rows.append(dict(hist=list(ids), P=P, n=n, min_new=min_new, table=table, N=N))
        prompts.append(ids[:P])
        settings.append((n, min_new, table))
    return rows, prompts, settings


def arm_state(rows, hist_ld, device="cpu"):
    """A ConstraintState holding ``rows`` (prompt + already generated ids) as the oracle sees them."""
    B = len(rows)
    st = fused_ops.ConstraintState(B, hist_ld, device)
    st.arm([r["hist"] for r in rows], [(r["n"], r["min_new"], r["table"]) for r in rows])
    st.prompt_len.copy_(torch.tensor([r["P"] for r in rows], dtype=torch.int32))
    return st


@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
def test_host_form_equals_oracle(dt):
    rng = random.Random({"f16": 16, "bf16": 61, "f32": 32}[dt])
    g = torch.Generator().manual_seed(7)
    for case in range(40):
        B, N, hist_ld = rng.choice([1, 3, 4]), rng.choice([1, 7, 40]), rng.choice([1, 6, 30])
        rows, _, _ = random_case(rng, B, N, hist_ld)
        st = arm_state(rows, hist_ld)
        with_rows = case % 2 == 0
        row_state = [[len(r["hist"]) - r["P"], CO.FINISHED if rng.random() < 0.2 else 0] for r in rows] if with_rows else None
        live = sum(1 for s in row_state if not s[1]) if with_rows else None
        rs_t = torch.tensor(row_state, dtype=torch.int32) if with_rows else None
        live_t = torch.tensor([live], dtype=torch.int32) if with_rows else None
        for step in range(3):
            x = (torch.randn(B, N, generator=g) * 3).to(DT[dt])
            bits = to_bits(x)
            tok = None if step == 0 else [rng.randrange(min(5, N)) for _ in range(B)]
            live = CO.launch(bits, dt, rows, hist_ld, tok, row_state, live)
            out = fused_ops.history_constraints(x, st, None if tok is None else torch.tensor(tok, dtype=torch.int64), rs_t, live_t)
            assert out is x
            assert np.array_equal(to_bits(x), bits), (dt, case, step)
            assert st.hist_len.tolist() == [len(r["hist"]) for r in rows]
            for b, r in enumerate(rows):
                assert st.hist[b, :len(r["hist"])].tolist() == r["hist"]
            if with_rows:
                assert rs_t.tolist() == row_state and int(live_t) == live


def test_host_form_out_of_range_ids_are_stored_and_ban_nothing():
    N = 6
    rows = [dict(hist=[-1, N, -1], P=1, n=2, min_new=0, table=[(BAN, [N, 3])], N=N)]
    st = arm_state(rows, 8)
    x = torch.zeros(1, N)
    fused_ops.history_constraints(x, st, torch.tensor([N], dtype=torch.int64))
    assert st.hist[0, :4].tolist() == [-1, N, -1, N] and torch.isinf(x[0]).nonzero().view(-1).tolist() == [3]
    x = torch.zeros(1, N)
    fused_ops.history_constraints(x, st, torch.tensor([-1], dtype=torch.int64))      # the 2-gram rule names N: outside, nothing banned
    assert st.hist[0, :5].tolist() == [-1, N, -1, N, -1] and not torch.isinf(x).any()


# ---- validation --------------------------------------------------------------------------------------------------------------------------
def test_check_argument_errors():
    C = fused_ops.ConstraintState
    SM, LM = fused_ops.CONSTRAINT_SEQS_MAX, fused_ops.CONSTRAINT_SEQ_LEN_MAX
    assert (SM, LM) == (32, 16)
    with pytest.raises(ValueError, match="CONSTRAINT_SEQS_MAX"):
        C.check(1, bad_words_ids=[[i] for i in range(SM + 1)])
    with pytest.raises(ValueError, match=str(SM)):
        C.check(1, bad_words_ids=[[i] for i in range(20)], stop_sequences=[[i, i] for i in range(12)], min_new_tokens=2, eos_id=3)
    with pytest.raises(ValueError, match="CONSTRAINT_SEQ_LEN_MAX"):
        C.check(1, stop_sequences=[list(range(LM + 1))])
    with pytest.raises(ValueError, match="CONSTRAINT_SEQ_LEN_MAX"):
        C.check(1, no_repeat_ngram_size=LM + 1)
    with pytest.raises(ValueError, match="empty"):
        C.check(1, bad_words_ids=[[1], []])
    with pytest.raises(ValueError, match="empty"):
        C.check(2, stop_sequences=[None, [[]]])
    for kw in (dict(no_repeat_ngram_size=-1), dict(min_new_tokens=-1), dict(no_repeat_ngram_size=1.5), dict(bad_words_ids=[[-1]]),
               dict(bad_words_ids=[[5]], vocab=5), dict(min_new_tokens=1, eos_id=9, vocab=9), dict(bad_words_ids=7),
               dict(bad_words_ids=[1, 2])):
        with pytest.raises(ValueError):
            C.check(1, **kw)
    for kw in (dict(no_repeat_ngram_size=None), dict(no_repeat_ngram_size="2"), dict(min_new_tokens=None), dict(min_new_tokens="x"),
               dict(no_repeat_ngram_size=True), dict(bad_words_ids=[["a"]]), dict(bad_words_ids=[[None]]), dict(min_new_tokens=1, eos_id="e")):
        with pytest.raises(ValueError, match="row 0"):           # a wrong type is a ValueError naming the row, never a TypeError
            C.check(1, **kw)
    # per-row forms: wrong lengths
    for kw in (dict(no_repeat_ngram_size=[1, 2, 3]), dict(min_new_tokens=[1]), dict(bad_words_ids=[None, [[1]], None]),
               dict(stop_sequences=[[[1, 2]]])):
        with pytest.raises(ValueError, match="for 2 rows"):
            C.check(2, **kw)
    with pytest.raises(ValueError, match="row 1"):
        C.check(2, no_repeat_ngram_size=[0, -3])
    # the caps themselves are fine; nesting depth decides between "every row" and "one per row"
    full = C.check(2, no_repeat_ngram_size=LM, bad_words_ids=[[i] for i in range(SM - 1)], min_new_tokens=4, eos_id=2)
    assert [len(t) for _, _, t in full] == [SM, SM] and full[0][2][-1] == (MIN, [2])
    a = C.check(2, bad_words_ids=[[1, 2], [3]], stop_sequences=[None, [[4, 5]]])
    assert a[0] == (0, 0, [(BAN, [1, 2]), (BAN, [3])]) and a[1] == (0, 0, [(BAN, [1, 2]), (BAN, [3]), (STOP, [4, 5])])
    assert C.neutral(C.check(3)) and C.neutral(C.check(2, min_new_tokens=5)) and C.neutral(C.check(1, bad_words_ids=[], stop_sequences=[None]))
    assert not C.neutral(C.check(2, no_repeat_ngram_size=[0, 1])) and not C.neutral(C.check(1, min_new_tokens=1, eos_id=0))
    st = C(2, 4, "cpu")
    with pytest.raises(ValueError):
        st.arm([[1, 2, 3, 4, 5], []], C.check(2, no_repeat_ngram_size=2))       # a prompt longer than the history
    with pytest.raises(ValueError):
        st.arm([[1]], C.check(1, no_repeat_ngram_size=2))
    with pytest.raises(ValueError):
        fused_ops.history_constraints(torch.zeros(3, 5), st)
    with pytest.raises(ValueError):
        fused_ops.history_constraints(torch.zeros(2, 5), st, row_state=torch.zeros(2, 2, dtype=torch.int32))   # no live


def test_declarations():
    header = open(os.path.join(ROOT, "include", "qlinear_hip.h")).read()
    assert re.search(r"^int qlinear_history_constraints\(", header, re.M)
    assert re.search(r"^#define QL_CONSTRAINT_SEQS_MAX 32$", header, re.M) and re.search(r"^#define QL_CONSTRAINT_SEQ_LEN_MAX 16$", header, re.M)
    assert re.search(r"^#define QLINEAR_ABI_VERSION 3$", header, re.M) and "Still 3: qlinear_history_constraints" in header
    assert "qlinear_history_constraints" in _lib.EXPORTS
    makefile = open(os.path.join(ROOT, "chatglm_q_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", makefile, re.M).group(1).split()
    assert "history_constraints.hip" in srcs and os.path.exists(os.path.join(ROOT, "chatglm_q_amd", "csrc", "history_constraints.hip"))


# ---- the tiny model, greedy --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_f32():
    return build("f32")


PROMPT, T = [17, 3, 99, 250, 8, 61], 24


def ngrams(ids, n):
    return [tuple(ids[i:i + n]) for i in range(len(ids) - n + 1)]


def has_repeat(ids, n):
    g = ngrams(ids, n)
    return len(set(g)) < len(g)


@pytest.fixture(scope="module")
def base(tiny_f32):
    model, cfg = tiny_f32
    dec = ChatGLMDecoder(cfg, model)
    out = list(dec.generate_ids(PROMPT, max_generated_tokens=T, greedy=True, ignore_eos=True))
    assert dec.last_stats["constraints"] is False and dec.last_stats["stop_sequence"] is None
    assert dec._session.con is None                              # never armed: nothing allocated
    return out


def test_no_repeat_ngram(tiny_f32, base):
    model, cfg = tiny_f32
    assert has_repeat(base, 2)                                   # the precondition: greedy decoding loops
    dec = ChatGLMDecoder(cfg, model)
    got = list(dec.generate_ids(PROMPT, max_generated_tokens=T, greedy=True, ignore_eos=True, no_repeat_ngram_size=2))
    assert len(got) == T and not has_repeat(got, 2) and not has_repeat(PROMPT + got, 2)
    assert dec.last_stats["constraints"] is True
    first = next(i for i in range(2, T + 1) if has_repeat(PROMPT + base[:i], 2))
    assert got[:first - 1] == base[:first - 1] and got[first - 1] != base[first - 1]   # unchanged up to the first repeat
    # the sampled path (the host decides) obeys the rule too
    torch.manual_seed(11)
    sampled = list(dec.generate_ids(PROMPT, max_generated_tokens=T, ignore_eos=True, no_repeat_ngram_size=2, temperature=0.3))
    assert len(sampled) == T and not has_repeat(PROMPT + sampled, 2)


def test_bad_words(tiny_f32, base):
    model, cfg = tiny_f32
    j = 3
    a, b = base[j], base[j + 1]
    assert (a, b) not in ngrams(PROMPT + base[:j + 1], 2)        # the precondition: position j is the bigram's first occurrence
    dec = ChatGLMDecoder(cfg, model)
    got = list(dec.generate_ids(PROMPT, max_generated_tokens=T, greedy=True, ignore_eos=True, bad_words_ids=[[a, b]]))
    assert got[:j + 1] == base[:j + 1] and got[j + 1] != b and (a, b) not in ngrams(PROMPT + got, 2)
    # a single id is banned everywhere, the prompt's last id counts as the head of a sequence
    one = list(dec.generate_ids(PROMPT, max_generated_tokens=T, greedy=True, ignore_eos=True, bad_words_ids=[[base[0]], [PROMPT[-1], base[1]]]))
    assert base[0] not in one and one != base
    first = list(dec.generate_ids(PROMPT, max_generated_tokens=4, greedy=True, ignore_eos=True, bad_words_ids=[[PROMPT[-1], base[0]]]))
    assert first[0] != base[0]


def test_stop_sequence(tiny_f32, base):
    model, cfg = tiny_f32
    j = 5
    stop = [base[j], base[j + 1]]
    assert tuple(stop) not in ngrams(base[:j + 1], 2)            # the precondition: the pair completes at j + 1 for the first time
    dec = ChatGLMDecoder(cfg, model)
    got = list(dec.generate_ids(PROMPT, max_generated_tokens=T, greedy=True, ignore_eos=True, stop_sequences=[stop]))
    assert got == base[:j + 2] and dec.last_stats["stop_sequence"] == 0 and dec.last_stats["constraints"] is True
    got = list(dec.generate_ids(PROMPT, max_generated_tokens=T, greedy=True, ignore_eos=True, stop_sequences=[[255, 254], stop, [base[j + 1]]]))
    assert got[-1] == base[j + 1] and dec.last_stats["stop_sequence"] in (1, 2) and len(got) <= j + 2
    # a sequence that straddles the prompt boundary does not stop; one that ends with the first token does
    got = list(dec.generate_ids(PROMPT, max_generated_tokens=T, greedy=True, ignore_eos=True, stop_sequences=[[PROMPT[-1], base[0]]]))
    assert got == base and dec.last_stats["stop_sequence"] is None
    got = list(dec.generate_ids(PROMPT, max_generated_tokens=T, greedy=True, ignore_eos=True, stop_sequences=[[base[0]]]))
    assert got == base[:1] and dec.last_stats["stop_sequence"] == 0
    # the loop in which the host reads nothing until the end is not taken with stop sequences
    got = list(dec.generate_ids(PROMPT, max_generated_tokens=T, greedy=True, ignore_eos=True, sync_every_token=False, stop_sequences=[stop]))
    assert got == base[:j + 2]


def test_min_new_tokens(tiny_f32, base):
    model, cfg = tiny_f32
    j = 2
    eos = base[j]
    assert eos not in base[:j]
    dec = ChatGLMDecoder(cfg, model, eos_token_id=eos)
    assert list(dec.generate_ids(PROMPT, max_generated_tokens=T, greedy=True)) == base[:j + 1]      # the precondition: it ends at j
    got = list(dec.generate_ids(PROMPT, max_generated_tokens=T, greedy=True, min_new_tokens=j + 3))
    assert len(got) >= j + 3 and eos not in got[:j + 3] and got[:j] == base[:j]
    assert dec.last_stats["constraints"] is True
    if len(got) < T:
        assert got[-1] == eos
    # without an end id there is nothing to hold back
    assert list(dec.generate_ids(PROMPT, max_generated_tokens=T, greedy=True, ignore_eos=True, min_new_tokens=9)) == base
    assert dec.last_stats["constraints"] is False


BATCH = [[5, 9, 200, 31, 7, 44, 3, 12], [44, 3], PROMPT, [100, 101, 102, 0], [1, 2, 3, 4]]


def test_generate_batch_ids_per_prompt(tiny_f32, base):
    model, cfg = tiny_f32
    dec = ChatGLMDecoder(cfg, model)
    kw = dict(max_generated_tokens=T, greedy=True, ignore_eos=True)
    plain = dec.generate_batch_ids(BATCH, **kw)
    assert dec.last_stats["constraints"] is False and dec.last_stats["stop_sequence"] == [None] * 5
    assert dec._batch_sessions[5][1].con is None
    assert plain[2] == base
    # row 0: no-repeat 2-grams; row 1: a banned bigram; row 2: defaults; row 3: a stop sequence; row 4: a banned single id
    assert has_repeat(plain[0], 2)
    j1 = next(i for i in range(1, T - 1) if (plain[1][i], plain[1][i + 1]) not in ngrams(BATCH[1] + plain[1][:i + 1], 2))
    bad = [plain[1][j1], plain[1][j1 + 1]]
    j3 = 4
    stop = [plain[3][j3], plain[3][j3 + 1]]
    assert tuple(stop) not in ngrams(plain[3][:j3 + 1], 2)
    got = dec.generate_batch_ids(BATCH, no_repeat_ngram_size=[2, 0, 0, 0, 0], bad_words_ids=[None, [bad], None, None, [[plain[4][0]]]],
                                 stop_sequences=[None, None, None, [[250, 251, 252], stop], None], **kw)
    assert dec.last_stats["constraints"] is True
    assert not has_repeat(BATCH[0] + got[0], 2) and len(got[0]) == T
    assert got[1][:j1 + 1] == plain[1][:j1 + 1] and got[1][j1 + 1] != bad[1] and tuple(bad) not in ngrams(BATCH[1] + got[1], 2)
    assert got[2] == plain[2]                                    # a row with defaults: its unconstrained tokens
    assert got[3] == plain[3][:j3 + 2]                           # ends with the sequence
    assert plain[4][0] not in got[4] and len(got[4]) == T
    assert dec.last_stats["stop_sequence"] == [None, None, None, 1, None] and dec.last_stats["generated"][3] == j3 + 2
    # each row equals generate_ids with the row's own settings
    one = ChatGLMDecoder(cfg, model)
    assert got[0] == list(one.generate_ids(BATCH[0], no_repeat_ngram_size=2, **kw))
    assert got[1] == list(one.generate_ids(BATCH[1], bad_words_ids=[bad], **kw))
    assert got[3] == list(one.generate_ids(BATCH[3], stop_sequences=[[250, 251, 252], stop], **kw))
    # a shared list applies to every row
    shared = dec.generate_batch_ids(BATCH, no_repeat_ngram_size=2, **kw)
    assert all(not has_repeat(p + o, 2) for p, o in zip(BATCH, shared)) and shared[0] == got[0]


def test_generate_batch_ids_min_new_tokens(tiny_f32, base):
    model, cfg = tiny_f32
    j = 2
    eos = base[j]
    dec = ChatGLMDecoder(cfg, model, eos_token_id=eos)
    kw = dict(max_generated_tokens=T, greedy=True)
    plain = dec.generate_batch_ids([PROMPT, PROMPT], **kw)
    assert plain == [base[:j + 1]] * 2                           # the precondition: both rows end at j
    got = dec.generate_batch_ids([PROMPT, PROMPT], min_new_tokens=[j + 3, 0], **kw)
    assert got[1] == base[:j + 1] and len(got[0]) >= j + 3 and eos not in got[0][:j + 3]
    solo = ChatGLMDecoder(cfg, model, eos_token_id=eos)
    assert got[0] == list(solo.generate_ids(PROMPT, min_new_tokens=j + 3, **kw))


def test_api_argument_errors(tiny_f32):
    model, cfg = tiny_f32
    dec = ChatGLMDecoder(cfg, model)
    for kw in (dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=17), dict(min_new_tokens=-2), dict(bad_words_ids=[[]]),
               dict(stop_sequences=[list(range(17))]), dict(bad_words_ids=[[cfg.vocab_size]]), dict(bad_words_ids=[[i] for i in range(33)]),
               dict(bad_words_ids=[[i] for i in range(20)], stop_sequences=[[i] for i in range(13)])):
        with pytest.raises(ValueError):
            list(dec.generate_ids([1, 2, 3], max_generated_tokens=4, greedy=True, **kw))
        with pytest.raises(ValueError):
            dec.generate_batch_ids([[1, 2], [3]], max_generated_tokens=4, greedy=True, **kw)
    for kw in (dict(no_repeat_ngram_size=[1]), dict(min_new_tokens=[1, 2, 3]), dict(bad_words_ids=[None, None, None]),
               dict(stop_sequences=[[[1]], None, [[2]]])):
        with pytest.raises(ValueError):
            dec.generate_batch_ids([[1, 2], [3]], max_generated_tokens=4, greedy=True, **kw)

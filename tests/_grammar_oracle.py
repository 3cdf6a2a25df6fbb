"""Oracle of the grammar mask (qlinear_grammar_mask, include/qlinear_hip.h): rules 0 - 3 restated in plain Python over a ``ByteDFA``'s raw
arrays and a list of byte strings, logits as integer bit patterns in numpy arrays.  Shares nothing with the host form in
chatglm_q_amd/fused_ops.py, with ``ByteDFA.step`` or with the kernel.  Also: the generator of the synthetic vocabularies the tests use."""
import random

import numpy as np

NEG_INF = {"f16": 0xFC00, "bf16": 0xFF80, "f32": 0xFF800000}
FINISHED = 1
DEAD = 0xFFFF


def walk(dfa, s, data):
    """The state after the bytes ``data`` from ``s``; -1 = dead, and dead stays dead."""
    if s < 0 or s >= dfa.n_states:
        return -1
    for v in data:
        t = int(dfa.table[s, int(dfa.class_of[v])])
        if t == DEAD:
            return -1
        s = t
    return s


def allowed_ids(dfa, s, vocab, eos, N):
    """The ids of [0, N) a row in state ``s`` may choose: a non-empty byte string the automaton survives; the end id exactly when ``s`` is
    live and accepting - and when ``s`` is dead, where nothing else is left."""
    out = set()
    for i in range(N):
        if i == eos:
            if s < 0 or dfa.accept[s]:
                out.add(i)
        elif i < len(vocab) and len(vocab[i]) > 0 and walk(dfa, s, vocab[i]) >= 0:
            out.add(i)
    return out


def advance(dfa, s, vocab, N, tok):
    """Rule 1: the state after the fed id; an id outside the table or with no bytes changes nothing."""
    if tok is None or not 0 <= tok < min(N, len(vocab)):
        return s if 0 <= s < dfa.n_states else -1
    return walk(dfa, s, vocab[tok])


def launch(bits, dt, rows, vocab, tok=None, row_state=None):
    """One launch.  ``bits`` (B, ld) unsigned: the logits' bit patterns, the first ``rows[b]["N"]`` columns of each row are logits;
    ``rows``: one dict per row - dfa (None: no grammar), state, eos (-1: none), N; ``tok``: B ids or None; ``row_state``: B [count, flags]
    lists or None.  ``bits`` and the rows' states are changed in place."""
    for b, r in enumerate(rows):
        if row_state is not None and row_state[b][1] & FINISHED:
            continue
        dfa = r["dfa"]
        if dfa is None:
            continue
        s = advance(dfa, r["state"], vocab, r["N"], None if tok is None else int(tok[b]))
        ok = allowed_ids(dfa, s, vocab, r["eos"], r["N"])
        for i in range(r["N"]):
            if i not in ok:
                bits[b, i] = NEG_INF[dt]
        r["state"] = s


def make_vocab(n, seed=0, singles=b"", alphabet=b"abcd019 -,.{}\":yesnoABCD", extra=()):
    """A synthetic vocabulary of ``n`` byte strings: first ``extra`` (given tokens), then every single byte of ``singles``, then random
    strings of 0 - 12 bytes over ``alphabet`` (about one in twelve empty), some with bytes >= 0x80 (whole UTF-8 characters and lone
    continuation bytes), and - from 64 tokens up - one 40-byte token.  Shuffled with the seed, so ids carry no order."""
    rng = random.Random(seed)
    toks = [bytes(t) for t in extra] + [bytes([v]) for v in dict.fromkeys(singles)]
    toks = toks[:n]
    high = ["é".encode(), "€".encode(), "好".encode(), "𝄞".encode(), b"\x80", b"\xbf\x80", "é€".encode()]
    while len(toks) < n:
        k = len(toks)
        if n >= 64 and k == n - 1:
            toks.append(bytes(rng.choice(alphabet) for _ in range(40)))
        elif k % 9 == 5:
            toks.append(rng.choice(high) + bytes(rng.choice(alphabet) for _ in range(rng.randrange(0, 3))))
        else:
            L = rng.choice([0, 1, 1, 1, 2, 2, 2, 3, 3, 4, 5, 6, 8, 12])
            toks.append(bytes(rng.choice(alphabet) for _ in range(L)))
    rng.shuffle(toks)
    return toks

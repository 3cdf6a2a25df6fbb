"""Oracle of the history constraints (qlinear_history_constraints, include/qlinear_hip.h): rules 0 - 3 restated with Python sets and
list slices on plain lists of ids, logits as integer bit patterns in numpy arrays.  Shares nothing with the host form in
chatglm_q_amd/fused_ops.py or with the kernel."""
import numpy as np

BAN, STOP, MIN = 0, 1, 2
SEQS_MAX, SEQ_LEN_MAX = 32, 16
NEG_INF = {"f16": 0xFC00, "bf16": 0xFF80, "f32": 0xFF800000}
BITS = {"f16": np.uint16, "bf16": np.uint16, "f32": np.uint32}
FINISHED = 1


def ngram_bans(h, n):
    """The Hugging Face no-repeat rule: the ids that would complete an n-gram the history already holds."""
    if n < 1:
        return set()
    L = len(h)
    return {h[i + n - 1] for i in range(L - n + 1) if h[i:i + n - 1] == h[L - n + 1:]}


def sequence_bans(h, P, table, min_new):
    """What the BAN and MIN entries of ``table`` ([(kind, ids), ...]) name for the history ``h`` whose first ``P`` ids are the prompt."""
    out, L = set(), len(h)
    for kind, q in table:
        m = len(q)
        if kind == BAN and L >= m - 1 and h[L - (m - 1):] == q[:-1]:
            out.add(q[-1])
        if kind == MIN and L - P < min_new:
            out.add(q[0])
    return out


def stop_index(h, P, table):
    """The smallest table index of a STOP entry that the GENERATED part of ``h`` ends with; None when there is none."""
    generated = h[P:]
    for s, (kind, q) in enumerate(table):
        if kind == STOP and len(q) <= len(generated) and generated[len(generated) - len(q):] == q:
            return s
    return None


def bans(h, P, n, min_new, table):
    return ngram_bans(h, n) | sequence_bans(h, P, table, min_new)


def launch(bits, dt, rows, hist_ld, tok=None, row_state=None, live=None):
    """One launch.  ``bits`` (B, ld) unsigned: the logits' bit patterns, N = ``rows[b]["N"]`` columns of each row are logits;
    ``rows``: one dict per row - hist (list), P, n, min_new, table; ``tok``: B ids or None; ``row_state``: B [count, flags] lists or
    None; ``live``: an int or None.  Everything is changed in place; returns ``live``."""
    for b, r in enumerate(rows):
        if row_state is not None and row_state[b][1] & FINISHED:
            continue
        h = r["hist"]
        if tok is not None and len(h) < hist_ld:
            h.append(int(tok[b]))
        if row_state is not None and stop_index(h, r["P"], r["table"]) is not None:
            row_state[b][1] |= FINISHED
            live -= 1
            continue
        for v in bans(h, r["P"], r["n"], r["min_new"], r["table"]):
            if 0 <= v < r["N"]:
                bits[b, v] = NEG_INF[dt]
    return live

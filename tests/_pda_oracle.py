"""Oracle of the pushdown automaton's mask (qlinear_pda_mask, include/qlinear_hip.h): rules 0 - 6 restated in plain Python over a
``BytePDA``'s raw arrays and a list of byte strings, the stack a plain list, logits as integer bit patterns in numpy arrays.  Shares
nothing with the host form in chatglm_q_amd/fused_ops.py, with ``BytePDA.step`` or with the kernel.

A row is a dict: pda (None: no grammar), state (-1: dead), depth, stack (64 symbols as the device holds them, bottom first), eos (-1:
none), N, and optionally n_states / n_syms / max_depth as the device's cfg holds them when a test has corrupted them."""
import numpy as np

NEG_INF = {"f16": 0xFC00, "bf16": 0xFF80, "f32": 0xFF800000}
FINISHED = 1
TABLE_MAX, STATES_MAX, DEPTH_MAX, LOCAL_MAX, SYMS_MAX = 16384, 4095, 64, 32, 3


def new_row(pda, eos, N, **over):
    return dict(pda=pda, state=0, depth=0, stack=[0] * DEPTH_MAX, eos=eos, N=N, **over)


class Machine:
    """Row constants behind the clamps of rule 6 and the moves of rules 2 and 3."""

    def __init__(self, row):
        pda = row["pda"]
        self.ns = min(row.get("n_states", pda.n_states), STATES_MAX)
        self.nsy = max(0, min(row.get("n_syms", pda.n_syms), SYMS_MAX))
        self.maxd = max(0, min(row.get("max_depth", pda.max_depth), DEPTH_MAX))
        self.cls = [int(c) for c in pda.class_of]
        self.nc = max(self.cls) + 1
        self.ns = min(self.ns, TABLE_MAX // ((self.nsy + 1) * self.nc))
        flat = [int(e) for e in pda.table.reshape(-1)]
        self.flat = flat + [0xFFFF] * (TABLE_MAX - len(flat))   # the row's table as armed: no move past the automaton's own entries
        self.accept = [int(a) for a in pda.accept]

    def valid(self, s, stack):
        return 0 <= s < self.ns and len(stack) <= self.maxd and (not stack or 1 <= stack[-1] <= self.nsy)

    def walk(self, s, stack, data):
        """(state, stack) after the bytes ``data`` of ONE token from a valid (s, stack); None = dead."""
        stack = list(stack)
        lowest = len(stack)
        for v in data:
            top = stack[-1] if stack else 0
            e = self.flat[(s * (self.nsy + 1) + top) * self.nc + self.cls[v]]
            nxt, op, sym = e & 0xFFF, (e >> 12) & 3, e >> 14
            if nxt >= self.ns or op == 3:
                return None
            if op == 1:
                if not stack:
                    return None
                stack.pop()
                lowest = min(lowest, len(stack))
                if stack and not 1 <= stack[-1] <= self.nsy:    # a corrupt symbol uncovered: dead
                    return None
            elif op == 2:
                if sym == 0 or sym > self.nsy or len(stack) == self.maxd:
                    return None
                stack.append(sym)
                if len(stack) - lowest > LOCAL_MAX:              # the window rule
                    return None
            s = nxt
        return s, stack


def token_of(vocab, N, i):
    return vocab[i] if 0 <= i < min(N, len(vocab)) else b""


def allowed_ids(m, config, vocab, eos, N):
    """The ids of [0, N) a row may choose from ``config`` ((state, stack) or None = dead)."""
    out = set()
    for i in range(N):
        if i == eos:
            if config is None or (m.accept[config[0]] and not config[1]):
                out.add(i)
        elif config is not None and len(token_of(vocab, N, i)) > 0 and m.walk(config[0], config[1], token_of(vocab, N, i)) is not None:
            out.add(i)
    return out


def launch(bits, dt, rows, vocab, tok=None, row_state=None):
    """One launch.  ``bits`` (B, ld) unsigned: the logits' bit patterns, the first ``rows[b]["N"]`` columns of each row are logits;
    ``tok``: B ids or None; ``row_state``: B [count, flags] lists or None.  ``bits`` and the rows are changed in place."""
    for b, r in enumerate(rows):
        if row_state is not None and row_state[b][1] & FINISHED:
            continue
        if r["pda"] is None or r.get("n_states", 1) <= 0:
            continue
        m = Machine(r)
        d = r["depth"]
        config = None
        if 0 <= d <= m.maxd and m.valid(r["state"], r["stack"][:d]):
            config = (r["state"], r["stack"][:d])
        lowest = d
        if config is not None and tok is not None:
            fed = token_of(vocab, r["N"], int(tok[b]))
            if fed:
                config = m.walk(config[0], config[1], fed)
                if config is not None:                          # the lowest depth the advance reached: the common prefix with the old stack
                    depth_at = [d]
                    s, st = r["state"], list(r["stack"][:d])
                    for v in fed:
                        s, st = m.walk(s, st, bytes([v]))
                        depth_at.append(len(st))
                    lowest = min(depth_at)
        ok = allowed_ids(m, config, vocab, r["eos"], r["N"])
        for i in range(r["N"]):
            if i not in ok:
                bits[b, i] = NEG_INF[dt]
        if config is None:
            r["state"] = -1                                      # a dead row keeps its depth and its stack bytes
        else:
            r["state"], r["depth"] = config[0], len(config[1])
            r["stack"][lowest:len(config[1])] = config[1][lowest:]


def device_rows(st, rows):
    """Copy the rows' state / depth / stack / cfg overrides into a ``fused_ops.PdaState`` armed with their automata."""
    import torch
    st.state.copy_(torch.tensor([r["state"] for r in rows], dtype=torch.int32))
    st.depth.copy_(torch.tensor([r["depth"] for r in rows], dtype=torch.int32))
    st.stack.copy_(torch.tensor([r["stack"] for r in rows], dtype=torch.uint8))
    cfg = st.cfg.cpu()
    for b, r in enumerate(rows):
        for k, name in ((0, "n_states"), (2, "n_syms"), (3, "max_depth")):
            if name in r:
                cfg[b, k] = r[name]
    st.cfg.copy_(cfg)
    return st


def assert_rows(st, rows):
    """The device's state, depth and stack against the rows' (every stack byte: entries the launch must not write keep theirs)."""
    assert st.state.cpu().tolist() == [r["state"] if r["pda"] is not None else 0 for r in rows]
    assert st.depth.cpu().tolist() == [r["depth"] for r in rows]
    assert st.stack.cpu().tolist() == [r["stack"] for r in rows]
    assert st.ticket.cpu().tolist() == [0] * len(rows)

"""The beam search rules in plain Python - the single source of truth for ``qlinear_beam_advance`` (csrc/beam_search.hip), its host form
(``fused_ops._beam_advance_host``) and ``ChatGLMDecoder.beam_search_ids``.  Every number is a numpy float32 and every operation one
correctly rounded fp32 add / divide / compare, so kernel, host form and oracle agree bit for bit.

P prompts x B beams = R rows; rows g*B .. g*B+B-1 are group g.  One ``advance`` is one generation step of every group:

  row candidates   per row the 2B best ids of its logits in ``step_logprobs``' order with their log-probs (the caller supplies them:
                   ``cand_ids`` / ``cand_lp`` (R, n) with n <= 2B entries per row)
  group merge      score = beam_score[row] + lp (one fp32 add); the group's candidates ordered by score descending (a NaN ranks as
                   -inf), then row ascending, then in-row rank ascending; the first 2B are walked
  walk             t = tokens generated after this step (1-based).  End id at merged rank < B: a finished hypothesis
                   (score / norm[t], t, parent row); end id at rank >= B: skipped; any other candidate: the next running beam, until
                   B are filled
  finished heap    B slots per group: append while fewer than B are held, otherwise replace the worst (lowest score, on ties the
                   highest slot) when the new score is strictly greater
  done             early_stopping: the heap holds B.  Otherwise: it holds B and its worst score >= best new running score / norm[t]
  done groups      (and groups whose trellis is full) ride along: tok = the end id (0 without one), parent = the row itself, nothing
                   else changes
  trellis          every step appends (token, parent row) per row at the group's step count
  budget end       ``finalize``: a group that is not done adds its running beams as hypotheses score / norm[t] under the same heap
                   rule; per prompt the hypotheses are sorted by score descending, then earlier finish step, then lower slot
"""
import numpy as np

F = np.float32
NEG_INF = F(-np.inf)


def norm_table(cap, length_penalty):
    """norm[len] = float32(float64(len) ** length_penalty) for len = 0 .. cap (0 ** a negative penalty: inf)."""
    lp = float(length_penalty)
    zero = 1.0 if lp == 0 else (0.0 if lp > 0 else float("inf"))
    return np.array([zero] + [float(n) ** lp for n in range(1, cap + 1)], dtype=np.float64).astype(np.float32)


def order_key(s):
    return NEG_INF if s != s else s


def fdiv(a, b):
    with np.errstate(all="ignore"):
        return F(F(a) / F(b))


def fadd(a, b):
    with np.errstate(all="ignore"):
        return F(F(a) + F(b))


def heap_add(heap, B, entry, events=None):
    """``heap``: list of at most B entries (score, ...), slot = list index.  Returns the slot written or None.  ``events``: a dict
    that counts what happened (the tests assert that their cases occur)."""
    def note(what):
        if events is not None:
            events[what] = events.get(what, 0) + 1
    if len(heap) < B:
        heap.append(entry)
        note("heap_append")
        return len(heap) - 1
    worst = worst_slot(heap)
    if entry[0] > heap[worst][0]:
        heap[worst] = entry
        note("heap_replace")
        return worst
    note("heap_keep_equal" if entry[0] == heap[worst][0] else "heap_keep_less")
    return None


def worst_slot(heap):
    worst = 0
    for s in range(1, len(heap)):
        if heap[s][0] <= heap[worst][0]:         # ties: the highest slot
            worst = s
    return worst


class Beams:
    def __init__(self, P, B, eos, length_penalty, early_stopping, cap):
        self.P, self.B, self.cap = P, B, cap
        self.eos = -1 if eos is None or eos < 0 else int(eos)
        self.early = bool(early_stopping)
        self.norm = norm_table(cap, length_penalty)
        self.score = [F(0) if r % B == 0 else NEG_INF for r in range(P * B)]
        self.steps = [0] * P
        self.done = [False] * P
        self.live = P
        self.heap = [[] for _ in range(P)]       # entries (score, t, parent row, sum_logprob)
        self.trellis = {}                        # (slot, row) -> (token, parent row)
        self.tok = [0] * (P * B)
        self.parent = list(range(P * B))
        self.events = {}                         # what the rules met so far: the tests assert that their cases occur

    def note(self, what):
        self.events[what] = self.events.get(what, 0) + 1

    def advance(self, cand_ids, cand_lp):
        """One step of every group from the rows' candidate lists; returns (tok, parent) of all R rows."""
        P, B = self.P, self.B
        for g in range(P):
            rows = range(g * B, g * B + B)
            if self.done[g] or self.steps[g] >= self.cap:
                for r in rows:
                    self.tok[r], self.parent[r] = (self.eos if self.eos >= 0 else 0), r
                self.note("ride_done" if self.done[g] else "ride_full")
                continue
            cands = []
            for r in rows:
                for k in range(len(cand_ids[r])):
                    s = fadd(self.score[r], cand_lp[r][k])
                    cands.append((s, r, k, int(cand_ids[r][k])))
            cands.sort(key=lambda c: (-float(order_key(c[0])), c[1], c[2]))
            if any(a[0] == b[0] and a[1] != b[1] for a, b in zip(cands[:2 * B], cands[1:2 * B + 1])):
                self.note("tie_across_rows")
            t = self.steps[g] + 1
            nrm = self.norm[t]
            nxt = []
            for j, (s, r, k, i) in enumerate(cands[:2 * B]):
                if self.eos >= 0 and i == self.eos:
                    if j < B:
                        heap_add(self.heap[g], B, (fdiv(s, nrm), t, r, s), self.events)
                    else:
                        self.note("end_skipped")
                    continue
                nxt.append((i, r, s))
                if len(nxt) == B:
                    break
            assert len(nxt) == B, "2B candidates always suffice"
            full = len(self.heap[g]) == B
            if self.early:
                done = full
            else:
                done = full and bool(self.heap[g][worst_slot(self.heap[g])][0] >= fdiv(nxt[0][2], nrm))
            for n, r in enumerate(rows):
                i, p, s = nxt[n]
                self.tok[r], self.parent[r], self.score[r] = i, p, s
                self.trellis[(self.steps[g], r)] = (i, p)
            self.steps[g] = t
            if done:
                self.done[g] = True
                self.live -= 1
                self.note("done")
        return list(self.tok), list(self.parent)

    def backtrack(self, row, slots):
        """The ids of the beam that sits in ``row`` after ``slots`` steps."""
        ids = []
        for s in range(slots - 1, -1, -1):
            tok, row = self.trellis[(s, row)]
            ids.append(tok)
        return ids[::-1]

    def finalize(self, num_return):
        """Per prompt the ``num_return`` best hypotheses as (ids, score, sum_logprob)."""
        out = []
        for g in range(self.P):
            B = self.B
            heap = [(e[0], e[1], e[2], e[3], True) for e in self.heap[g]]
            if not self.done[g] and self.steps[g] > 0:
                t = self.steps[g]
                for r in range(g * B, g * B + B):
                    heap_add(heap, B, (fdiv(self.score[r], self.norm[t]), t, r, self.score[r], False))
            order = sorted(range(len(heap)), key=lambda s: (-float(order_key(heap[s][0])), heap[s][1], s))
            hyps = []
            for s in order[:num_return]:
                score, t, row, total, ended = heap[s]
                ids = self.backtrack(row, t - 1) + [self.eos] if ended else self.backtrack(row, t)
                hyps.append((ids, score, total))
            out.append(hyps)
        return out

"""Token-by-token decode loop around the quantized model (harness for BASELINE configs 4 and 5).

Counterpart of the reference's ``ChatGLMDecoder.generate`` and ``top_p_sampling``
(chatglm_q/decoder.py:12-27,65-108): batch 1, same sampler, same timing definitions
(``gen = (n - 1) / sum(t[1:])``, ``avg = n / sum(t)``, chatglm_q/decoder.py:99-106).

MI355X-first differences (results unchanged):
  * the key/value cache is preallocated and a decode step is shape-static, so ONE step - 113 QLinear
    launches plus the small ops around them - is captured in a HIP graph and replayed per token; the
    position counter, the cache write index, the attention mask, the choice of the next token - the
    reference's top-k / top-p sampler (``qlinear_top_p_sample``: one launch, counter-based generator in
    device memory) or the argmax - and the next input id are all updated on the device inside that
    graph, so the host only replays it;
  * lm_head is evaluated for the last position only (the loop uses nothing else, decoder.py:85);
  * prefill can be chunked (`prefill_chunk`), each chunk one forward over batch x chunk rows.
Text handling (tokenizer, chat template, punctuation fix-ups) is out of scope: the loop works on token ids;
a tokenizer object with ``encode`` / ``decode`` may be supplied and is used if present.
"""
from __future__ import annotations

import time
from typing import Iterable, NamedTuple, Optional

import torch
from torch import Tensor

from .model import ChatGLM2Model, KVCache


def top_p_sampling(logits: Tensor, top_k: int = 100, top_p: float = 0.8, temperature: float = 1.0) -> Tensor:
    """softmax(logits / T) -> keep the top_k most likely -> drop those whose preceding cumulative mass
    exceeds top_p -> renormalise -> one multinomial draw (chatglm_q/decoder.py:12-27)."""
    probs = torch.softmax(logits.float() / temperature, dim=-1)
    probs, indices = torch.sort(probs, dim=-1, descending=True)
    probs, indices = probs[..., :top_k], indices[..., :top_k]
    before = torch.cumsum(probs, dim=-1) - probs
    probs = torch.where(before > top_p, torch.zeros_like(probs), probs)
    probs = probs / probs.sum(dim=-1, keepdim=True)
    pick = torch.multinomial(probs, num_samples=1)
    return torch.gather(indices, dim=-1, index=pick)[..., 0]


def filtered_distribution(logits: Tensor, top_k: int = 100, top_p: float = 0.8, temperature: float = 1.0):
    """The deterministic part of the sampler: (renormalised probabilities, token indices)."""
    probs = torch.softmax(logits.float() / temperature, dim=-1)
    probs, indices = torch.sort(probs, dim=-1, descending=True)
    probs, indices = probs[..., :top_k], indices[..., :top_k]
    before = torch.cumsum(probs, dim=-1) - probs
    probs = torch.where(before > top_p, torch.zeros_like(probs), probs)
    return probs / probs.sum(dim=-1, keepdim=True), indices


# The logit stages of a decode step, in launch order, between lm_head and the selection ("The step plan"): the tag of the graph
# key, the session attribute that holds the stage's state, its ``fused_ops`` function (looked up through the module at call time) and
# whether the call also takes ``rows.live`` (the history constraints finish rows on their stop sequences).
LOGIT_STAGES = (
    ("pen", "pen", "logit_penalties", False),
    ("con", "con", "history_constraints", True),
    ("gr", "gr", "grammar_mask", False),
    ("pda", "pda", "pda_mask", False),
)


class StepPlan(NamedTuple):
    """Which launches make up one decode step behind lm_head, in order: the logit ``stages`` (tags of LOGIT_STAGES), the selection of
    ``selector`` - "logits" (the host decides), "greedy", "sample", "rows" or "beam" - and, with ``lp``, the log-prob record's.  ``key``
    names the captured graph: "greedy", "sample+pen", "rows+pen+con+gr+lp", ...  A "beam" step has neither stages nor record.  A
    "logits" step launches neither and its key is bare: ``stages`` / ``lp`` then say what the caller applies to the logits it gets back."""
    selector: str
    stages: tuple
    lp: bool
    key: str

    @property
    def in_step(self) -> tuple:
        """The stages the step itself launches."""
        return () if self.selector == "logits" else self.stages


_PLANS: dict = {}


def step_plan(greedy: bool = True, sample: bool = False, rows: bool = False, pen: bool = False, lp: bool = False, con: bool = False,
              beam: bool = False, gr: bool = False, pda: bool = False) -> StepPlan:
    """The plan of the step ``DecodeSession.capture`` / ``decode_step`` are asked for with these flags (memoised: one lookup per step).
    ``beam`` wins over the other selectors, ``rows`` over ``sample`` over ``greedy``."""
    flags = (greedy, sample, rows, pen, lp, con, beam, gr, pda)
    plan = _PLANS.get(flags)
    if plan is None:
        selector = "beam" if beam else "rows" if rows else "sample" if sample else "greedy" if greedy else "logits"
        on = dict(pen=pen, con=con, gr=gr, pda=pda)
        stages = tuple(tag for tag, _, _, _ in LOGIT_STAGES if on[tag])
        if selector == "beam":                                  # the beam search's step: no sampling controls, no record
            plan = StepPlan(selector, (), False, selector)
        elif selector == "logits":                              # the host decides: it adjusts and records what it gets back
            plan = StepPlan(selector, stages, bool(lp), selector)
        else:                                                   # "greedy+pen", "sample+lp", "rows+pen+con+gr+lp", ...: graphs of their own
            plan = StepPlan(selector, stages, bool(lp), "+".join((selector,) + stages + (("lp",) if lp else ())))
        _PLANS[flags] = plan
    return plan


# hook of the developer experiments (chatglm_q_amd/dev/experiments.py); None in the product
AHEAD_LAUNCH = True           # greedy graph decoding launches step k + 1 before reading token k (ChatGLMDecoder._generate)
POST_GENERATE_CHECK = None

class ScoreResult:
    """What ``DecodeSession.score`` returns.  ``logprobs`` (batch, S - 1) fp32: entry t is log p(labels[:, t + 1] | ids[:, :t + 1]),
    0 where that label is -100; ``valid`` (batch, S - 1) bool: which entries were scored; ``loss``: 0-dim fp32, minus the mean of
    the scored entries (the reference's ``F.cross_entropy`` mean, chatglm_q/model.py:388); ``argmax`` (batch, S - 1) int64 or
    None: the model's own choice at every position; ``logits`` (batch, vocab): the last position's, as ``prefill`` returns them."""
    __slots__ = ("logprobs", "valid", "loss", "argmax", "logits")

    def __init__(self, logprobs: Tensor, valid: Tensor, loss: Tensor, argmax: Optional[Tensor], logits: Tensor):
        self.logprobs, self.valid, self.loss, self.argmax, self.logits = logprobs, valid, loss, argmax, logits


class GenerationLogprobs:
    """What a generation with ``logprobs=n`` leaves in ``ChatGLMDecoder.last_logprobs`` for one sequence, one entry per token
    returned: ``token_logprobs[t]`` = log p(token t | everything before it) under the logits the selection read (after penalties
    and bias, before temperature / top-k / top-p); ``top_ids[t]`` / ``top_logprobs[t]`` = the n most likely ids at that step (most
    likely first, ties: lowest id first) and their log-probs."""
    __slots__ = ("token_logprobs", "top_ids", "top_logprobs")

    def __init__(self, token_logprobs, top_ids, top_logprobs):
        self.token_logprobs, self.top_ids, self.top_logprobs = token_logprobs, top_ids, top_logprobs

    def __len__(self):
        return len(self.token_logprobs)

    def __repr__(self):
        return f"GenerationLogprobs({len(self)} tokens, {len(self.top_ids[0]) if self.top_ids else 0} alternatives)"


class BeamHypothesis:
    """One result of ``ChatGLMDecoder.beam_search_ids``: ``ids`` - the generated ids (ending with the end token when the hypothesis
    finished on it); ``score`` - ``sum_logprob / len(ids) ** length_penalty``, what the hypotheses are ranked by; ``sum_logprob`` - the
    sum of the ids' log-probs under the model."""
    __slots__ = ("ids", "score", "sum_logprob")

    def __init__(self, ids, score, sum_logprob):
        self.ids, self.score, self.sum_logprob = ids, score, sum_logprob

    def __repr__(self):
        return f"BeamHypothesis({len(self.ids)} tokens, score {self.score:.6g})"


def check_logprobs(logprobs) -> Optional[int]:
    """``logprobs`` of generate_ids / generate_batch_ids: None = off, an int in [0, TOP_LOGPROBS_MAX] = that many alternatives."""
    from .fused_ops import TOP_LOGPROBS_MAX
    if logprobs is None:
        return None
    if isinstance(logprobs, bool) or not isinstance(logprobs, int) or not 0 <= logprobs <= TOP_LOGPROBS_MAX:
        raise ValueError(f"logprobs must be None or an int in [0, {TOP_LOGPROBS_MAX}] (got {logprobs!r})")
    return int(logprobs)


def matched_stop_sequence(ids, stop_sequences) -> Optional[int]:
    """Index of the first of ``stop_sequences`` (lists of ids) that ``ids`` ends with; None when it ends with none of them."""
    for s, q in enumerate(stop_sequences):
        if 0 < len(q) <= len(ids) and list(ids[len(ids) - len(q):]) == list(q):
            return s
    return None


class DecodeSession:
    """One sequence batch on one device: preallocated cache, eager (chunked) prefill, graph-replayed decode."""

    def __init__(self, model: ChatGLM2Model, batch: int, capacity: int, use_graph: Optional[bool] = None,
                 decode_only: bool = False, low_footprint: bool = False):
        self.model = model
        # low_footprint (round 5): once the derived layouts a phase reads exist, the canonical GPU buffers of every int4 module are
        # dropped (DynamicQuantizeLinear.drop_canonical: state_dict() / save_pretrained rebuild them byte for byte from part 1) -
        # ChatGLM2-6B int4g32: ~8.5 GB resident for prefill + decode, ~3.5 GB with decode_only (the reference's "6G+", readme.md:72)
        self.low_footprint = low_footprint
        # decode_only: before the decode step is captured, free the derived layouts only prefill / batched rows use (part 2 of
        # every int4 layer, the un-gated part 1 of w_in once its gate-interleaved copy exists): ~10.8 -> ~6.6 GB resident for
        # ChatGLM2-6B int4g32.  A later prefill rebuilds what it needs (and the graph is re-captured).
        self.decode_only = decode_only
        p = model.final_ln.weight
        self.device, self.dtype = p.device, p.dtype
        if capacity > model.config.max_sequence_length:
            raise ValueError(f"cache capacity {capacity} exceeds max_sequence_length {model.config.max_sequence_length} "
                             "(no rotary table rows for those positions)")
        self.batch, self.capacity = batch, capacity
        self.cache: KVCache = model.new_cache(batch, capacity)
        self.use_graph = (self.device.type == "cuda") if use_graph is None else use_graph
        dev = self.device
        # device-resident step state (static addresses: the captured graph reads and updates them)
        self.tok = torch.zeros(batch, 1, dtype=torch.long, device=dev)
        self.write_index = torch.zeros(1, dtype=torch.long, device=dev)
        self.pos = torch.zeros(batch, 1, dtype=torch.long, device=dev)
        self.mask = torch.full((batch, 1, capacity), -1e10, dtype=torch.float32, device=dev)
        self.pad_cols = torch.zeros(batch, capacity, dtype=torch.bool, device=dev)   # left-padding columns (never attended)
        self.n_tokens = torch.zeros(batch, dtype=torch.long, device=dev)             # real tokens per sequence so far
        self.logits: Optional[Tensor] = None
        self.graph = None                                       # the captured step of the mode last asked for ...
        self._graphs = {}                                       # ... of every mode captured under the current layouts
        self._graph_logits = {}                                 # ... and the logits buffer each of them writes (every graph has its own)
        self._captured_mode = None
        self._graph_key = None
        # the device sampler's state (chatglm_q/decoder.py:12-27 inside the captured step): top_k / top_p / temperature and the
        # generator's (seed, per-row draw counter) live in device memory, so one captured graph serves every setting and every seed
        self.sample_params = torch.tensor([100.0, 0.8, 1.0], dtype=torch.float32, device=dev)
        self.rng_state = torch.zeros(1 + batch, dtype=torch.long, device=dev)
        # the batched generation's per-row state (arm_rows): sampler settings, generators, token counts / flags, budgets, the tokens
        # themselves and the live-row count, read and updated on the device by the "rows" step
        from .fused_ops import BatchRows
        self.rows = BatchRows(batch, capacity, dev)
        self._rows_stop = None                                  # the stop id the captured "rows" step bakes in
        # sampling controls (arm_penalties): token history, penalties and logit bias in device memory, read and updated by the
        # "+pen" steps.  Allocated by the first penalised generation: a session that never uses them holds nothing extra
        self.pen = None
        # the record of the "+lp" steps (arm_logprobs): every generated token's log-prob and the most likely alternatives, appended
        # on the device and read once at the end.  Allocated by the first generation that asks for log-probs
        self.lp = None
        # history constraints (arm_constraints): every row's ordered token history and its no-repeat / banned / stop / minimum-length
        # settings in device memory, read and updated by the "+con" steps.  Allocated by the first constrained generation
        self.con = None
        # regex-constrained generation (arm_grammar): the vocabulary's byte table, every row's automaton and its current state in device
        # memory, read and advanced by the "+gr" steps.  Allocated by the first generation with a grammar
        self.gr = None
        self._gr_source = None                                  # the TokenBytes the GrammarState was built from
        # JSON-constrained generation (arm_grammar, when a row's grammar is a grammar.BytePDA): the same with a stack beside every row's
        # state, read and advanced by the "+pda" steps - which then serve the call's DFA rows too.  Allocated by the first such generation
        self.pda = None
        self._pda_source = None
        # beam search (arm_beams): beam scores, parents, the trellis and the finished heaps in device memory, read and updated by the
        # "beam" step, and the table of cache buffers its gather reorders.  Allocated by the first beam search
        self.beams = None
        self._beam_table = None
        self._beams_B = None                                    # the beam count the captured "beam" step bakes in
        self.length = 0
        self.busy = False                                       # a generate_ids generator is running on this session

    def reset(self):
        """Forget the sequences (not the captured graph): the session can serve the next generation.  Cache rows need no
        clearing - every position is masked until a prefill / decode step writes and unmasks it."""
        self.length = 0
        self.cache.length = 0
        self.pad_cols.zero_()
        self.n_tokens.zero_()
        self.write_index.zero_()
        self.pos.zero_()
        self.mask.fill_(-1e10)
        return self

    # -- prefill -------------------------------------------------------------------------------------
    @torch.no_grad()
    def prefill(self, ids: Tensor, chunk: Optional[int] = None, attention_mask: Optional[Tensor] = None) -> Tensor:
        """ids (batch, S).  Returns the last position's logits (batch, vocab).

        ``attention_mask`` (batch, S), 1 = token / 0 = pad, follows the reference's convention for batches of unequal
        length (chatglm_q/model.py:297-318): sequences are LEFT padded, a pad column is masked for every query
        (``causal | ~attention_mask``) and a token's rotary position is its count among the real tokens
        (``cumsum(attention_mask)``: 1-based, pads get 0).  The pad columns stay masked through later chunks and
        decode steps."""
        return self._prefill(ids, chunk, attention_mask, None)

    def _prefill(self, ids: Tensor, chunk: Optional[int], attention_mask: Optional[Tensor], per_chunk) -> Tensor:
        """The chunked loop behind ``prefill`` and ``score``.  ``per_chunk`` None: lm_head runs for every chunk's last position
        only.  Otherwise every chunk's hidden states in front of ``final_ln`` go to ``per_chunk(s0, s1, hidden)`` and the last
        position's logits are formed from the final chunk's."""
        B, S = ids.shape
        if S + self.length > self.capacity:
            raise ValueError(f"sequence {S + self.length} exceeds the cache capacity {self.capacity}")
        ids = ids.to(self.device)
        if attention_mask is None:
            valid = torch.ones(B, S, dtype=torch.bool, device=self.device)
        else:
            if attention_mask.shape != ids.shape:
                raise ValueError(f"attention_mask {tuple(attention_mask.shape)} != ids {tuple(ids.shape)}")
            valid = attention_mask.to(self.device).bool()
        self.pad_cols[:, self.length:self.length + S] = ~valid
        positions = self.n_tokens[:, None] + torch.cumsum(valid.long(), dim=1)       # 1-based among real tokens
        positions = torch.where(valid, positions, torch.zeros_like(positions))       # cumsum of a left pad is 0
        # default: the whole prompt in one pass while that is at most 8192 rows per QLinear call (where the prefill GEMMs are at their
        # best and the (batch, chunk, keys) mask stays small), otherwise chunks of 8192 // batch positions
        chunk = chunk or (S if B * S <= 8192 else max(256, 8192 // B))
        t = torch.arange(self.capacity, device=self.device)
        logits = None
        for s0 in range(0, S, chunk):
            s1 = min(S, s0 + chunk)
            rows = torch.arange(self.length + s0, self.length + s1, device=self.device)
            blocked = (t[None, None, :] > rows[None, :, None]) | self.pad_cols[:, None, :]
            mask = blocked.float() * -1e10
            if per_chunk is None:
                logits = self.model.step(ids[:, s0:s1], self.cache, rows, positions[:, s0:s1], mask,
                                         last_only=True, kv_len=self.length + s1)
            else:
                hidden = self.model.step(ids[:, s0:s1], self.cache, rows, positions[:, s0:s1], mask,
                                         kv_len=self.length + s1, return_hidden=True)
                del mask, blocked
                per_chunk(s0, s1, hidden)
                if s1 == S:
                    logits = self.model.head(hidden[:, -1:])
                del hidden
        self.length += S
        self.cache.length = self.length
        self.n_tokens += valid.long().sum(dim=1)
        # arm the decode-step state
        self.write_index.fill_(self.length)
        self.pos.copy_((self.n_tokens + 1)[:, None])            # positions are 1-based (model.py:308)
        self.mask.fill_(-1e10)
        self.mask[:, :, : self.length + 1] = 0.0                # incl. the position the next step writes
        self.mask.masked_fill_(self.pad_cols[:, None, :], -1e10)
        if self.low_footprint:
            self.drop_canonical()                               # the layouts this prefill read exist now: the canonical copies can go
        return logits[:, -1]

    # -- scoring -------------------------------------------------------------------------------------
    def default_head_rows(self) -> int:
        """Rows of logits ``score`` holds at a time when not told otherwise: a block of at most 256 MiB, at most 2048 rows
        (2048 rows at vocabulary 65024 in a 16-bit dtype)."""
        row_bytes = self.model.config.vocab_size * torch.empty((), dtype=self.dtype).element_size()
        return max(1, min(2048, (256 << 20) // row_bytes))

    @torch.no_grad()
    def score(self, ids: Tensor, attention_mask: Optional[Tensor] = None, labels: Optional[Tensor] = None,
              chunk: Optional[int] = None, head_rows: Optional[int] = None, return_argmax: bool = False) -> "ScoreResult":
        """Per-token log-probabilities of given ids on the prefill path: the reference's ``forward(labels=...)``
        (chatglm_q/model.py:384-390) and its perplexity run (examples/evaluations/ppl.py) without ever holding the
        (batch, S, vocab) logits.  ids (batch, S), ``attention_mask`` as in ``prefill`` (left padding).  ``labels`` (batch, S)
        follow the reference's convention - same alignment as ids, no shift, -100 = not scored - and default to ``ids`` with
        -100 at the pad positions (the reference tokenizer's ``return_labels``, chatglm_q/tokenizer.py:138-142): position t
        is scored against ``labels[:, t + 1]``.

        The same chunked loop as ``prefill`` (``chunk``); per chunk, ``final_ln`` + ``lm_head`` run over blocks of at most
        ``head_rows`` rows (default: ``default_head_rows()``) and each block of logits goes through one
        ``fused_ops.token_logprob`` launch and is dropped.  Nothing in the loop waits for the device.  Afterwards the session is
        armed exactly as after ``prefill(ids)``: ``decode_step`` continues the sequences, ``ScoreResult.logits`` are the last
        position's logits as ``prefill`` returns them.

        An entry whose QUERY position is a pad - with the default labels, the one in front of a padded row's first token - is
        scored as the reference scores it, from a position whose attention row is masked everywhere and therefore averages every
        key of the forward pass: it equals the reference's one-pass ``forward`` when the ids go through in one chunk and moves
        with ``chunk`` (as the reference's own forward with ``past_key_values`` does).  Every other entry is a function of its
        sequence alone.  ``ChatGLMDecoder.score_ids`` leaves those entries out unless asked."""
        from . import fused_ops
        B, S = ids.shape
        dev = self.device
        if labels is None:
            labels = ids.to(dev)
            if attention_mask is not None:
                labels = torch.where(attention_mask.to(dev).bool(), labels, torch.full_like(labels, -100))
        else:
            if labels.shape != ids.shape:
                raise ValueError(f"labels {tuple(labels.shape)} != ids {tuple(ids.shape)}")
            labels = labels.to(dev)
        if labels.dtype != torch.int64:
            labels = labels.long()
        head_rows = int(head_rows) if head_rows else self.default_head_rows()
        if head_rows < 1:
            raise ValueError("head_rows must be positive")
        # position t's target is labels[:, t + 1]; the last position has none (known up front: chunk / block boundaries need no care)
        targets = torch.cat((labels[:, 1:], torch.full((B, 1), -100, dtype=torch.int64, device=dev)), dim=1)
        logprobs = torch.zeros(B, S, dtype=torch.float32, device=dev)
        argmax = torch.zeros(B, S, dtype=torch.int64, device=dev) if return_argmax else None

        def per_chunk(s0, s1, hidden):
            h2 = hidden.reshape(B * (s1 - s0), hidden.shape[-1])           # row b * (s1 - s0) + (t - s0)
            tg = targets[:, s0:s1].reshape(-1)
            lps, ams = [], []
            for r0 in range(0, h2.shape[0], head_rows):
                block = self.model.head(h2[r0:r0 + head_rows])               # (rows, vocab): the only logits alive
                out = fused_ops.token_logprob(block, tg[r0:r0 + head_rows], -100, return_argmax=return_argmax)
                del block
                if return_argmax:
                    lps.append(out[0]); ams.append(out[1])
                else:
                    lps.append(out)
            logprobs[:, s0:s1] = torch.cat(lps).view(B, s1 - s0)
            if return_argmax:
                argmax[:, s0:s1] = torch.cat(ams).view(B, s1 - s0)

        last = self._prefill(ids, chunk, attention_mask, per_chunk)
        valid = targets[:, :-1] != -100
        lp = logprobs[:, :-1]
        loss = (-(lp.sum(dtype=torch.float64) / valid.sum())).float()       # F.cross_entropy's mean over the scored targets
        return ScoreResult(lp, valid, loss, argmax[:, :-1] if return_argmax else None, last)

    # -- one decode step -------------------------------------------------------------------------------
    def set_sampling(self, top_k: int = 100, top_p: float = 0.8, temperature: float = 1.0, seed: Optional[int] = None):
        """Arm the device sampler: its parameters and (seed given) a fresh generator state - draw counters back to 0."""
        if top_k < 1 or not temperature > 0:
            raise ValueError("top_k >= 1 and temperature > 0")
        self.sample_params.copy_(torch.tensor([float(top_k), float(top_p), float(temperature)], dtype=torch.float32))
        if seed is not None:
            st = torch.zeros(1 + self.batch, dtype=torch.long)
            st[0] = int(seed) & 0x7FFFFFFFFFFFFFFF
            self.rng_state.copy_(st)

    def device_sampler_serves(self, top_k: int) -> bool:
        """The one-launch sampler runs on a GPU for top_k <= 1024 (or a vocabulary that small); otherwise the composed torch ops."""
        from . import fused_ops
        return self.device.type == "cuda" and (top_k <= fused_ops.SAMPLER_MAX_TOP_K
                                               or self.model.config.vocab_size <= fused_ops.SAMPLER_MAX_TOP_K)

    def arm_penalties(self, prompts, repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, logit_bias=None) -> bool:
        """Arm the sampling controls for a new generation (``fused_ops.PenaltyState.arm``): ``prompts`` = the REAL prompt ids of
        every row (no pads); each setting is a scalar or one value per row, ``logit_bias`` a dict ``{id: value}`` (or None) or one
        per row.  Returns whether anything changes a logit; with every setting at its default nothing is armed - and nothing
        allocated - and the generation takes the unpenalised steps."""
        from . import fused_ops
        B = self.batch

        def per_row(name, v):
            return fused_ops.per_row(name, v, B, "arm_penalties")

        if len(prompts) != B:
            raise ValueError(f"arm_penalties: {len(prompts)} prompts for {B} rows")
        settings = list(zip(per_row("repetition_penalty", repetition_penalty), per_row("presence_penalty", presence_penalty),
                            per_row("frequency_penalty", frequency_penalty)))
        biases = per_row("logit_bias", logit_bias)
        vocab = self.model.config.vocab_size
        checked = fused_ops.PenaltyState.check(B, vocab, settings, biases)
        if fused_ops.PenaltyState.neutral(*checked):
            if self.pen is not None:
                self.pen.active = False
            return False
        if self.pen is None:
            self.pen = fused_ops.PenaltyState(B, vocab, self.device)
        self.pen.arm(prompts, settings, biases)
        return True

    def _apply_stages(self, stages, logits: Tensor, tok: Optional[Tensor], rows: bool = False) -> Tensor:
        """Launch the logit stages with these tags on `logits` (batch, vocab), in place and in LOGIT_STAGES' order: ``tok`` = the ids the
        step was fed (None: the first token after a prefill - nothing is counted, appended or walked), ``rows``: the batched
        generation's rows (finished ones are left alone).  Returns the adjusted logits."""
        from . import fused_ops
        lg = logits if logits.stride(-1) == 1 else logits.contiguous()
        row_state, live = (self.rows.row_state, self.rows.live) if rows else (None, None)
        for tag, attr, fn, takes_live in LOGIT_STAGES:
            if tag in stages:
                getattr(fused_ops, fn)(lg, getattr(self, attr), tok, row_state, *((live,) if takes_live else ()))
        return lg

    def first_logits(self, plan: StepPlan, logits: Tensor) -> Tensor:
        """The plan's logit stages applied in place to a prefill's last-position logits, in front of the first selection: nothing is
        generated yet, so the penalties see the prompt ids and the bias only, the constraints the bans the prompt alone decides, and
        every automaton stays at its start."""
        return self._apply_stages(plan.stages, logits, None, plan.selector == "rows")

    def host_logits(self, plan: StepPlan, logits: Tensor) -> Tensor:
        """The host-sampled mode: the plan's logit stages applied in place to the logits ``decode_step`` returned - ``tok`` holds the id
        that step was fed - in front of the host's own sampler."""
        return self._apply_stages(plan.stages, logits, self.tok.view(-1))

    def penalize_first(self, logits: Tensor, rows: bool = False) -> Tensor:
        """The armed sampling controls applied in place to a prefill's last-position logits (nothing generated yet: no count)."""
        return self._apply_stages(("pen",), logits, None, rows)

    def arm_constraints(self, prompts, no_repeat_ngram_size=0, bad_words_ids=None, stop_sequences=None, min_new_tokens=0,
                        eos_id=None, checked=None) -> bool:
        """Arm the history constraints for a new generation (``fused_ops.ConstraintState.arm``): ``prompts`` = the REAL prompt ids
        of every row (no pads); ``no_repeat_ngram_size`` / ``min_new_tokens`` a scalar or one value per row, ``bad_words_ids`` /
        ``stop_sequences`` a list of id lists (or None) or one such list per row; ``eos_id``: the id ``min_new_tokens`` holds back
        (None: ``min_new_tokens`` arms nothing).  Returns whether anything is armed; with every control at its default nothing is
        armed - and nothing allocated - and the generation takes the unconstrained steps.  ``checked``: the settings as
        ``ConstraintState.check`` has already returned them for this batch (a caller that validated up front); the other arguments are
        not looked at then."""
        from . import fused_ops
        B = self.batch
        if len(prompts) != B:
            raise ValueError(f"arm_constraints: {len(prompts)} prompts for {B} rows")
        settings = checked if checked is not None else fused_ops.ConstraintState.check(
            B, no_repeat_ngram_size, bad_words_ids, stop_sequences, min_new_tokens, eos_id, vocab=self.model.config.vocab_size)
        if len(settings) != B:
            raise ValueError(f"arm_constraints: {len(settings)} settings for {B} rows")
        if fused_ops.ConstraintState.neutral(settings):
            if self.con is not None:
                self.con.active = False
            return False
        if self.con is None:
            self.con = fused_ops.ConstraintState(B, self.capacity, self.device)
        self.con.arm(prompts, settings)
        return True

    def constrain_first(self, logits: Tensor, rows: bool = False) -> Tensor:
        """The armed history constraints applied in place to a prefill's last-position logits (nothing generated yet: nothing is
        appended) - behind ``penalize_first``, in front of the first selection."""
        return self._apply_stages(("con",), logits, None, rows)

    def arm_grammar(self, grammars, eos_id=None, token_bytes=None) -> bool:
        """Arm the grammars for a new generation (``fused_ops.GrammarState.arm``): ``grammars`` = one ``grammar.ByteDFA`` / pattern string /
        None for every row, or one per row (None: the row is unconstrained); ``eos_id``: the id a row may choose exactly when its
        output is a full match (one, or one per row; None: none).  ``token_bytes`` (``grammar.TokenBytes``): the vocabulary's byte
        table - needed by the first armed generation, kept afterwards; a different one replaces the buffers and drops the "+gr" graphs.
        With a ``grammar.BytePDA`` among the rows the same goes for ``self.pda`` (``fused_ops.PdaState.arm``) and the "+pda" graphs.
        Every state starts at 0.  Returns whether any row has a grammar; with none nothing is armed - and nothing allocated - and the
        generation takes the steps without the launch."""
        from . import fused_ops
        from .grammar import BytePDA, as_grammar
        B = self.batch
        dfas = [None if g is None else as_grammar(g) for g in fused_ops.ConstraintState.per_row("grammar", grammars, B)]
        if self.gr is not None:
            self.gr.active = False
        if self.pda is not None:
            self.pda.active = False
        if all(d is None for d in dfas):
            return False
        # one pushdown row: the whole call takes the "+pda" launch, every row's grammar goes into ``self.pda`` (a ``ByteDFA`` lifted by
        # ``BytePDA.from_dfa``) and ``self.gr`` stays as it is and is not launched
        tag, cls = ("pda", fused_ops.PdaState) if any(isinstance(d, BytePDA) for d in dfas) else ("gr", fused_ops.GrammarState)
        vocab = self.model.config.vocab_size
        automata, eos = cls.check(B, dfas, eos_id, vocab=vocab)
        state = getattr(self, tag)
        if token_bytes is None and state is None:
            raise ValueError("arm_grammar: a grammar needs the vocabulary's byte table (token_bytes=, grammar.token_byte_table builds one)")
        if state is None or (token_bytes is not None and token_bytes is not getattr(self, f"_{tag}_source")):
            if state is not None:                               # other buffers: the graphs that baked the old ones in go
                self._drop_graphs(lambda key: "+" + tag in key)
            table = token_bytes.padded(vocab) if len(token_bytes) < vocab else token_bytes   # a padded vocabulary's extra ids are empty
            state = cls(B, table, self.device)
            setattr(self, tag, state)
            setattr(self, f"_{tag}_source", token_bytes)
        state.arm(automata, eos)
        return True

    def grammar_stage(self, armed: bool) -> dict:
        """The step keywords of what the last ``arm_grammar`` (which returned ``armed``) armed: the pushdown launch ("+pda") in the
        DFA launch's ("+gr") place when a row's grammar is a ``BytePDA``."""
        pda = bool(armed) and self.pda_armed
        return dict(gr=bool(armed) and not pda, pda=pda)

    def _drop_graphs(self, predicate) -> None:
        """Forget the captured steps whose key ``predicate`` accepts (something they baked in has changed)."""
        for key in [k for k in self._graphs if predicate(k)]:
            self._graphs.pop(key, None)
            self._graph_logits.pop(key, None)
        if self._captured_mode is not None and predicate(self._captured_mode):
            self.graph = self._captured_mode = None

    @property
    def pda_armed(self) -> bool:
        """Whether the last ``arm_grammar`` armed the pushdown launch ("+pda") rather than the DFA launch ("+gr")."""
        return self.pda is not None and self.pda.active

    def pda_first(self, logits: Tensor, rows: bool = False) -> Tensor:
        """``grammar_first`` of the pushdown launch: the armed automata applied in place to a prefill's last-position logits (nothing
        generated yet: every configuration stays at its start)."""
        return self._apply_stages(("pda",), logits, None, rows)

    def grammar_first(self, logits: Tensor, rows: bool = False) -> Tensor:
        """The armed grammars applied in place to a prefill's last-position logits (nothing generated yet: every state stays at its
        start) - behind ``constrain_first``, in front of the first selection."""
        return self._apply_stages(("gr",), logits, None, rows)

    def arm_logprobs(self, on: bool = True) -> bool:
        """Arm the log-prob record for a new generation (``fused_ops.StepLogprobs``: allocated on first use, one entry per cache
        position, TOP_LOGPROBS_MAX alternatives wide) - nothing recorded yet.  ``on`` False: nothing is armed or allocated and the
        generation takes the steps without the record's launch.  Returns ``on``."""
        if not on:
            return False
        if self.lp is None:
            from . import fused_ops
            self.lp = fused_ops.StepLogprobs(self.batch, self.capacity, self.device)
        self.lp.arm()
        return True

    def logprobs_first(self, logits: Tensor, rows: bool = False) -> None:
        """Record the first token after a prefill: the eager launch behind ``sample_first`` / ``sample_rows_first`` / the host's
        choice, once ``tok`` holds the id, on the prefill's last-position logits (after ``penalize_first``)."""
        from . import fused_ops
        fused_ops.step_logprobs(logits, self.tok.view(-1), self.lp, self.rows.row_state if rows else None)

    def sample_first(self, logits: Tensor) -> Tensor:
        """The token after a prefill, drawn by the device sampler from the prefill's last-position logits (no bookkeeping: prefill
        armed the step state).  Returns the (batch,) device tensor; ``tok`` holds it as the next step's input."""
        from . import fused_ops
        lg = logits if logits.stride(-1) == 1 else logits.contiguous()
        fused_ops.top_p_sample(lg, self.tok.view(-1), self.rng_state, dev_params=self.sample_params)
        return self.tok.view(-1)

    def arm_beams(self, num_beams: int, eos_id: Optional[int] = None, length_penalty: float = 1.0, early_stopping: bool = True,
                  first: int = 0):
        """Arm a beam search over this session's rows (``fused_ops.BeamState.arm``: allocated on first use): ``batch / num_beams``
        prompts x ``num_beams`` beams, rows g * num_beams ... are prompt g's and must be prefilled with the same left-padded prompt;
        ``first`` = the prompt length, the first cache position a step's gather moves.  The captured "beam" step bakes the beam count
        in: a different one drops it."""
        from . import fused_ops
        B = int(num_beams)
        if not 1 <= B <= fused_ops.BEAMS_MAX or self.batch % B:
            raise ValueError(f"arm_beams: num_beams in [1, {fused_ops.BEAMS_MAX}] dividing the batch of {self.batch} (got {num_beams})")
        if self.model.config.vocab_size < 2 * B:
            raise ValueError(f"arm_beams: a vocabulary of {self.model.config.vocab_size} supplies no {2 * B} candidates per row")
        if self.beams is None:
            self.beams = fused_ops.BeamState(self.batch, self.capacity, self.device)
            self._beam_table = fused_ops.BeamGatherTable(list(self.cache.k) + list(self.cache.v))
        self.beams.arm(self.batch // B, B, eos_id, length_penalty, early_stopping, first)
        if self._beams_B is not None and self._beams_B != B:
            self._drop_graphs(lambda key: key == "beam")
            self._beams_B = None
        return self.beams

    def beam_first(self, logits: Tensor) -> None:
        """The first token of every beam after a prefill (no bookkeeping: prefill armed the step state): the candidates of the
        prefill's last-position logits, the selection (only a group's first row carries a finite score, so its 2B best ids seed the
        beams) and, once, the broadcast of every group's first row over the prompt positions [0, S) to its other rows - the step's
        gather never moves them again."""
        from . import fused_ops
        st = self.beams
        lg = logits if logits.stride(-1) == 1 else logits.contiguous()
        fused_ops.step_logprobs(lg, self.tok.view(-1), st.cand)
        fused_ops.beam_advance(st, self.tok.view(-1))
        lead = (torch.arange(self.batch, dtype=torch.int32) // st.B * st.B).to(self.device)
        fused_ops.beam_gather(self._beam_table, lead, torch.zeros(1, dtype=torch.int32, device=self.device), self.write_index, st.B)

    def arm_rows(self, params, seeds, budgets, stop_id: Optional[int] = None):
        """Arm the batched generation's per-row state (``fused_ops.BatchRows.arm``): one (top_k, top_p, temperature), seed and
        budget per row, and the stop id (None: none).  The captured "rows" step bakes the stop id in: a different one drops it."""
        self.rows.arm(params, seeds, budgets, stop_id)
        if self._rows_stop is not None and self._rows_stop != self.rows.stop_id:
            self._drop_graphs(lambda key: key.startswith("rows"))   # "rows", "rows+pen", "rows+con+lp", "rows+pen+lp", ...
            self._rows_stop = None

    def sample_rows_first(self, logits: Tensor) -> None:
        """The first token of every row after a prefill, selected and recorded by the batched step's kernel without bookkeeping
        (prefill armed the step state); ``tok`` holds the next step's input."""
        from . import fused_ops
        fused_ops.batch_sample_advance(logits, self.tok.view(-1), self.rows)

    def _step_body(self, plan: StepPlan):
        # invariant on entry: mask is 0 for positions <= write_index (the new position may attend to itself)
        from . import fused_ops
        logits = self.model.step(self.tok, self.cache, self.write_index, self.pos, self.mask, last_only=True)[:, -1]
        tok = self.tok.view(-1)
        if plan.selector == "beam":                             # candidates, cross-beam selection + bookkeeping, cache reorder: three launches
            st = self.beams
            fused_ops.step_logprobs(logits, tok, st.cand)
            fused_ops.beam_advance(st, tok, self.write_index, self.pos.view(-1), self.mask)
            fused_ops.beam_gather(self._beam_table, st.parent, st.first, self.write_index, st.B)
            return
        rows = plan.selector == "rows"
        # one launch per stage on the id this step was fed, the logits adjusted in place, in front of the selection (the host-decides
        # mode adjusts what it gets back)
        logits = self._apply_stages(plan.in_step, logits, tok, rows)
        if rows:                                                # per-row selection, recording, stop + the bookkeeping: one launch;
            # the tokens live in rows.out_tokens (self.logits is not touched)
            fused_ops.batch_sample_advance(logits, tok, self.rows, self.write_index, self.pos.view(-1), self.mask)
        else:
            self.logits = logits
            if plan.selector == "sample":                       # the reference's sampler + the bookkeeping: one launch
                logits = logits if logits.stride(-1) == 1 else logits.contiguous()
                fused_ops.top_p_sample(logits, tok, self.rng_state, dev_params=self.sample_params,
                                       write_index=self.write_index, pos=self.pos.view(-1), mask=self.mask)
            elif plan.selector == "greedy" and logits.is_cuda and logits.stride(-1) == 1:
                fused_ops.greedy_advance(logits, self.tok, self.write_index, self.pos, self.mask)   # one launch
            else:
                if plan.selector == "greedy":
                    self.tok.copy_(logits.argmax(dim=-1, keepdim=True))
                self.write_index.add_(1)
                self.pos.add_(1)
                self.mask.index_fill_(2, torch.clamp(self.write_index, max=self.capacity - 1), 0.0)
        if plan.lp and plan.selector != "logits":               # the record's launch, directly behind the selection (CPU: the host form)
            fused_ops.step_logprobs(logits, tok, self.lp, self.rows.row_state if rows else None)

    def drop_canonical(self) -> int:
        """Low-footprint mode: free the canonical buffers of every int4 module that can serve without them, and the plain copies of a
        first MLP projection that its gate-interleaved copies have made redundant (the fused step and the gated prefill GEMM read the
        gated part 1 / part 2; anything that asks for the plain ones again rebuilds them from what stays).  Returns the bytes freed."""
        freed = 0
        for m in self.model.modules():
            if not hasattr(m, "drop_canonical"):
                continue
            freed += m.drop_canonical()
            nb = m.derived_nbytes()
            parts = [plain for plain, gated in (("packed", "gated"), ("tiled", "gated_tiled")) if nb.get(plain) and nb.get(gated)]
            if parts and m.canonical_dropped:
                freed += sum(nb[k] for k in parts)
                m.release(*parts)
        return freed

    def release_prefill_layouts(self) -> int:
        """Free the derived layouts a one-row decode step never reads; returns the bytes released."""
        freed = 0
        for m in self.model.modules():
            if not (hasattr(m, "release") and hasattr(m, "derived_nbytes")):
                continue
            nb = m.derived_nbytes()
            parts = [k for k in ("tiled", "gated_tiled") if nb.get(k)]
            if nb.get("gated") and nb.get("packed") and "gated_tiled" in nb:      # int4 first MLP projection: the fused step reads the gated copy
                parts.append("packed")
            if parts:
                freed += sum(nb[k] for k in parts)
                m.release(*parts)
        return freed

    def _layout_fingerprint(self):
        """What a captured step bakes in besides this session's own buffers: the canonical buffers' identity + version and the
        derived layouts' addresses of every quantized module, and which path (``act_quant``) each one takes.  A graph captured
        under another fingerprint would replay against freed / stale derived buffers (``load_state_dict`` /
        ``apply_weights_`` / ``invalidate()`` drop them, the next forward allocates new ones) - ADVICE r2."""
        from . import _lib
        key = []
        for m in self.model.modules():
            if hasattr(m, "weight_scale") and hasattr(m, "weight"):
                derived = tuple(None if t is None else (t[0] if isinstance(t, tuple) else t).data_ptr()
                                for t in (getattr(m, a, None) for a in ("_packed", "_tiled", "_gated", "_gated_tiled", "_a8")))
                key.append((_lib.buffer_key(m.weight, m.weight_scale, getattr(m, "bias", None)), derived,
                            getattr(m, "act_quant", None)))
        return tuple(key)

    @property
    def _captured_greedy(self):                                 # kept for the developer tools that read it
        return self._captured_mode == "greedy"

    @torch.no_grad()
    def capture(self, greedy: bool = True, sample: bool = False, rows: bool = False, pen: bool = False, lp: bool = False,
                con: bool = False, beam: bool = False, gr: bool = False, pda: bool = False):
        """Capture one decode step of the plan these flags ask for (``step_plan``; DESIGN.md, "The step plan", lists the selectors, the
        stages, their order and the graph keys) - or keep the captured one while nothing it bakes in has changed.  Graphs of several
        plans live side by side under their keys (a decoder that alternates greedy and sampled generations captures each once); tables
        and states are device memory, so one graph serves every setting.  Every state a flag names must be armed first."""
        self._capture(step_plan(greedy, sample, rows, pen, lp, con, beam, gr, pda))

    # what arms each stage's state: named by the error of a capture that comes before it
    _ARMED_BY = {"pen": "arm_penalties", "con": "arm_constraints", "gr": "arm_grammar", "pda": "arm_grammar with a BytePDA"}

    def _capture(self, plan: StepPlan):
        if not self.use_graph:
            return
        from . import _lib
        mode, rows, beam = plan.key, plan.selector == "rows", plan.selector == "beam"
        lp = plan.lp and plan.selector != "logits"
        if beam and (self.beams is None or self.beams.B < 1):
            raise RuntimeError("capture(beam=True) before arm_beams")
        stage_states = [(tag, getattr(self, attr)) for tag, attr, _, _ in LOGIT_STAGES if tag in plan.in_step]
        for tag, st in stage_states:
            if st is None:
                raise RuntimeError(f"capture({tag}=True) before {self._ARMED_BY[tag]}")
        if lp and self.lp is None:
            raise RuntimeError("capture(lp=True) before arm_logprobs")
        if self._graphs:
            # cheap test first (a process-wide counter every derived-layout build / drop bumps), the full fingerprint when it moved
            valid = self._graph_epoch == _lib.layout_epoch() and self._graph_versions == self._canonical_versions()
            if not valid and self._graph_key == self._layout_fingerprint():
                self._graph_epoch, self._graph_versions = _lib.layout_epoch(), self._canonical_versions()
                valid = True
            if not valid:
                self._graphs.clear()                            # weights / layouts moved under the graphs: re-capture
                self._graph_logits.clear()
                self.graph = self._captured_mode = None
            elif mode in self._graphs:
                self._bind(mode)                                # a reused session keeps its graphs (static addresses)
                return
        if self.decode_only:
            self.release_prefill_layouts()
        # (the token counts of the sampling controls included: the warm-up runs must not count tokens; and the log-prob record's
        # entry counts: they must record nothing - what they wrote past the count is overwritten by the steps that follow; and the
        # history constraints' lengths: they must append nothing that survives - a row they stop comes back with row_state / live; and
        # the grammars' states: the warm-up runs must not walk them)
        state = (self.tok, self.write_index, self.pos, self.mask, self.rng_state) + self.rows.tensors()
        for _, st in stage_states:
            state += st.tensors()
        state += ((self.lp.count,) if lp else ()) + (self.beams.tensors() + (self.beams.first,) if beam else ())
        saved = tuple(t.clone() for t in state)
        if beam:
            # the warm-up's gathers touch only cache positions its own steps write, [write_index now, write_index then): every one of
            # them is written again by a real step before it is read, whatever the parents of the warm-up are
            self.beams.first.copy_(self.write_index.to(torch.int32))
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side):
            self._step_body(plan)                               # warm-up: allocations, lazy repacks
            # the warm-up built what the step reads (e.g. the gate-interleaved copy of w_in): what it made redundant goes now,
            # and the step runs once more so that every pre-bound launch exists before the capture
            if self.decode_only and self.release_prefill_layouts():
                self._step_body(plan)
            if self.low_footprint and self.drop_canonical():
                self._step_body(plan)                           # the pre-bound launches re-validate against the stand-in buffers
        torch.cuda.current_stream(self.device).wait_stream(side)
        if self._graphs and self._graph_epoch != _lib.layout_epoch():
            self._graphs.clear()                                # this mode's warm-up rebuilt / dropped a layout the older graphs baked in
            self._graph_logits.clear()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            self._step_body(plan)
        # capture ran the body twice on live state: restore (the cache rows it touched get rewritten)
        for dst, src in zip(state, saved):
            dst.copy_(src)
        if rows:
            self._rows_stop = self.rows.stop_id
        if beam:
            self._beams_B = self.beams.B
        self._graphs[mode] = graph
        # every graph writes a logits buffer of its own: kept with the graph and bound again whenever its mode comes back
        # ("rows" steps do not publish theirs)
        self._graph_logits[mode] = None if rows or beam else self.logits
        self.graph, self._captured_mode = graph, mode
        self._graph_key = self._layout_fingerprint()            # AFTER the warm-up built the lazy layouts
        self._graph_epoch, self._graph_versions = _lib.layout_epoch(), self._canonical_versions()

    def _bind(self, mode: str):
        """Make ``mode``'s captured step the current one: its graph and the logits buffer that graph writes."""
        self.graph, self._captured_mode = self._graphs[mode], mode
        if self._graph_logits.get(mode) is not None:
            self.logits = self._graph_logits[mode]

    def _canonical_versions(self):
        """Sum of the canonical buffers' version counters: moves on every in-place write autograd's bookkeeping sees
        (``copy_`` from a loader) even when no derived layout has been rebuilt yet."""
        total = 0
        for m in self.model.modules():
            if hasattr(m, "weight_scale") and hasattr(m, "weight"):
                for t in (m.weight, m.weight_scale, getattr(m, "bias", None)):
                    if t is not None:
                        try:
                            total += t._version
                        except RuntimeError:
                            pass
        return total

    @torch.no_grad()
    def decode_step(self, token: Optional[Tensor] = None, greedy: bool = True, sample: bool = False, rows: bool = False,
                    pen: bool = False, lp: bool = False, con: bool = False, beam: bool = False, gr: bool = False,
                    pda: bool = False) -> Tensor:
        """Advance by one token: one step of the plan these flags ask for (``step_plan``; DESIGN.md, "The step plan").  `token`
        (batch, 1) overrides the device-resident next id (needed when the host samples).  Returns this step's last-position logits
        (batch, vocab) - in the host-decides mode (neither greedy, sample nor rows) as the model gave them: the caller applies the
        stages and the record itself (``host_logits``, ``fused_ops.step_logprobs``) - or None for the "rows" and "beam" steps, whose
        tokens are in ``rows.out_tokens`` / ``beams``."""
        if self.length + 1 > self.capacity:
            raise ValueError("cache capacity exhausted")
        if token is not None:
            self.tok.copy_(token.to(self.device))
        plan = step_plan(greedy, sample, rows, pen, lp, con, beam, gr, pda)
        if plan.key in self._graphs:
            from . import _lib
            if self._graph_epoch != _lib.layout_epoch() or self._captured_mode != plan.key:   # a derived layout was rebuilt / dropped since
                self._capture(plan)                             # the capture: _capture() compares the fingerprint and keeps the graphs
            self.graph.replay()                                 # when only modules of OTHER models / sessions moved
        else:
            self._step_body(plan)
        self.length += 1
        self.cache.length = self.length
        return None if plan.selector in ("rows", "beam") else self.logits


class SentencePieceIds:
    """Token ids the way the reference's tokenizer produces them (chatglm_q/tokenizer.py:24-64), nothing else: the sentencepiece
    vocabulary followed by the five special tokens, ``encode`` = "[gMASK]" "<sop>" + pieces, ``decode`` drops every id past the
    sentencepiece vocabulary, ``tok[name]`` resolves special tokens and pieces.  The chat template and the punctuation fix-ups of
    the reference's text pipeline are out of scope."""
    SPECIAL = ("[MASK]", "[gMASK]", "[sMASK]", "<sop>", "<eop>")

    def __init__(self, model_file):
        import sentencepiece
        self.model_file = str(model_file)
        self.sp = sentencepiece.SentencePieceProcessor(model_file=self.model_file)
        self.n_pieces = len(self.sp)

    def __len__(self):
        return self.n_pieces + len(self.SPECIAL)

    def __getitem__(self, token: str) -> int:
        if token in self.SPECIAL:
            return self.n_pieces + self.SPECIAL.index(token)
        pid = self.sp.piece_to_id(token)
        if pid == self.sp.unk_id() and self.sp.id_to_piece(pid) != token:
            raise KeyError(token)
        return pid

    def encode(self, text: str, add_special_tokens: bool = True):
        ids = list(self.sp.encode(text))
        return [self["[gMASK]"], self["<sop>"]] + ids if add_special_tokens else ids

    def decode(self, ids) -> str:
        return self.sp.decode([int(i) for i in ids if int(i) < self.n_pieces])


def tok_file_of(tokenizer):
    """The sentencepiece file a tokenizer object was built from, when it says so (this module's wrapper: ``model_file``; the
    reference's ChatGLM2Tokenizer: ``vocab_file``)."""
    for attr in ("model_file", "vocab_file"):
        f = getattr(tokenizer, attr, None)
        if f is not None:
            return f
    return None


def _existing(p):
    return p if p.exists() else None


class ChatGLMDecoder:
    def __init__(self, config, model: ChatGLM2Model, tokenizer=None, eos_token_id: Optional[int] = None, device=None,
                 max_sequence_length: Optional[int] = None, time_log: bool = False, low_footprint: bool = False, token_bytes=None):
        # token_bytes (grammar.TokenBytes, or anything grammar.token_byte_table takes): every token's bytes, what ``grammar=`` walks;
        # None: built from the tokenizer's sentencepiece file by the first generation with a grammar
        self.token_bytes = token_bytes
        # low_footprint: the decoder's sessions drop the canonical GPU buffers of every int4 module once the derived layouts a phase
        # reads exist (DecodeSession(low_footprint=True): state_dict() / save_pretrained rebuild them byte for byte)
        self.low_footprint = low_footprint
        self.config = config
        self.model = model
        self.tokenizer = tokenizer
        self.device = device
        self.eos_token_id = eos_token_id
        self.max_sequence_length = max_sequence_length or model.config.max_sequence_length
        self.time_log = time_log
        self.last_stats: dict = {}
        # what the last generation with ``logprobs=n`` recorded: one GenerationLogprobs (generate_ids) or a list of them in prompt
        # order (generate_batch_ids); None after a generation without
        self.last_logprobs = None

    @staticmethod
    def from_pretrained(path, device=None, torch_dtype=None, tokenizer=None, eos_token: str = "</s>", time_log: bool = False,
                        low_footprint: Optional[bool] = None):
        """A reference-format checkpoint folder (``config.json`` + safetensors shards, chatglm_q/loader.py:69-110) -> a decoder
        whose ``generate`` / ``generate_ids`` run this build's fused path by default: preallocated cache, 5 launches per layer,
        one HIP graph per token on a GPU (chatglm_q/decoder.py:49-58 is the reference's constructor of the same name; the hub
        download it falls back to needs a network and is not offered).  ``device`` defaults to the GPU when there is one.
        ``tokenizer``: any object with ``encode`` / ``decode``; when omitted and the folder's sentencepiece file can be read, a
        plain SentencePiece wrapper is used (the reference's chat markers and punctuation fix-ups are text handling, out of scope).
        ``low_footprint`` (None = yes on a GPU): a decoder loaded for generation keeps ONE copy of every int4 weight per consumer -
        the canonical buffers are dropped once the derived layouts exist and rebuilt byte for byte when ``save_pretrained`` /
        ``state_dict()`` ask for them: ChatGLM2-6B int4g32 resident 7.1 GB (prefill + decode layouts) instead of 11.85 GB; the reference's
        guidance is "6G+" (readme.md:72); ``DecodeSession(decode_only=True, low_footprint=True)`` goes to 3.4 GB for decode-only serving."""
        from pathlib import Path
        from .loader import load_model
        path = Path(path)
        if not path.is_dir():
            raise FileNotFoundError(f"{path}: not a checkpoint folder (hub ids are not resolved: no network access in this build)")
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        config, model = load_model(path, torch_dtype, device)
        model.eval()
        eos_id = None
        tokenizer_path = None
        if tokenizer is None:
            tok_file = path / config.tokenizer_file
            if tok_file.exists():
                try:
                    tokenizer = SentencePieceIds(tok_file)
                except (ImportError, OSError, RuntimeError) as e:   # no sentencepiece module / unreadable or corrupt model file
                    # (sentencepiece raises RuntimeError on a file it cannot parse): the decoder still serves token ids
                    import warnings
                    warnings.warn(f"{tok_file}: no tokenizer built ({e}); generate() takes and yields token ids only")
                else:
                    tokenizer_path = tok_file
                    try:
                        eos_id = tokenizer[eos_token]
                    except KeyError:
                        eos_id = None
        elif hasattr(tokenizer, "__getitem__"):
            try:
                eos_id = tokenizer[eos_token]               # the reference tokenizer's lookup (chatglm_q/decoder.py:44)
            except (KeyError, TypeError):
                eos_id = None
        if low_footprint is None:
            low_footprint = torch.device(device).type == "cuda"
        dec = ChatGLMDecoder(config, model, tokenizer, eos_token_id=eos_id, device=device,
                             max_sequence_length=config.model_config.max_sequence_length, time_log=time_log, low_footprint=low_footprint)
        dec.tokenizer_file = tokenizer_path if tokenizer_path is not None else (tok_file_of(tokenizer) or _existing(path / config.tokenizer_file))
        return dec

    def save_pretrained(self, path, shard: bool = True, tokenizer_file=None):
        """chatglm_q/decoder.py:60-61: the folder ``from_pretrained`` (here or in the reference) reads back - ``config.json``, the
        safetensors shards and the sentencepiece file (``tokenizer_file``, default: the one ``from_pretrained`` loaded from; the
        reference's loader opens it unconditionally, chatglm_q/loader.py:85-88).  Without one the folder holds the model only and
        a warning says so."""
        from .loader import ChatGLMLoadConfig, save_model
        if not isinstance(self.config, ChatGLMLoadConfig):
            raise TypeError("save_pretrained needs the ChatGLMLoadConfig the decoder was built with")
        tok = tokenizer_file if tokenizer_file is not None else getattr(self, "tokenizer_file", None)
        if tok is None:
            import warnings
            warnings.warn("save_pretrained: no tokenizer file known (pass tokenizer_file=): the folder will hold the model only and the "
                          "reference's load_model_and_tokenizer will not open it")
        save_model(path, self.config, self.model, shard=shard, tokenizer_file=tok)

    def _grammar_table(self):
        """The vocabulary's byte table a grammar walks: ``token_bytes=`` of the constructor, or built once from the tokenizer."""
        from .grammar import TokenBytes, token_byte_table
        if self.token_bytes is None:
            if self.tokenizer is None:
                raise ValueError("grammar: the decoder has neither token_bytes= nor a tokenizer to build the vocabulary's byte table from")
            self.token_bytes = token_byte_table(self.tokenizer)
        elif not isinstance(self.token_bytes, TokenBytes):
            self.token_bytes = token_byte_table(self.token_bytes)
        return self.token_bytes

    def _grammar_result(self, dfa, ids, eos):
        """``last_stats["grammar_state"]`` of one row: "accepted" - the row ended on the end token and its bytes are a full match -
        "open" - the budget ran out inside the pattern - or None without a grammar.  Walked on the host over the ids handed out."""
        if dfa is None:
            return None
        ended = bool(ids) and eos is not None and ids[-1] == eos
        from .grammar import PDA_LOCAL_MAX, BytePDA
        if isinstance(dfa, BytePDA):                            # token by token, as the launch walks it (the window rule is per token)
            table, config = self._grammar_table(), dfa.start
            for i in (ids[:-1] if ended else ids):
                config = dfa.step(config, table.join([i]), window=PDA_LOCAL_MAX)
            return "accepted" if ended and dfa.accepting(config) else "open"
        state = dfa.step(0, self._grammar_table().join(ids[:-1] if ended else ids))
        return "accepted" if ended and dfa.accepting(state) else "open"

    def _session_for(self, capacity: int, use_graph: Optional[bool], batch: int = 1) -> DecodeSession:
        """One DecodeSession (cache + captured HIP graph) per batch size is kept and reused while the requested capacity fits and
        the model's parameters have not moved; a generation (batch 1: ``_session``) or a scoring call (``score_ids``: any batch)
        then costs no allocation and no re-capture."""
        p = self.model.final_ln.weight
        key = (p.device, p.dtype, p.data_ptr(), use_graph)
        if batch != 1:
            kept = self.__dict__.setdefault("_batch_sessions", {})
            sess = kept.get(batch)
            if sess is not None and sess[0] == key and sess[1].capacity >= capacity and not sess[1].busy:
                return sess[1].reset()
            new = DecodeSession(self.model, batch, capacity, use_graph, low_footprint=self.low_footprint)
            if sess is None or not sess[1].busy:
                kept[batch] = (key, new)
            return new
        sess = getattr(self, "_session", None)
        if sess is not None and self._session_key == key and sess.capacity >= capacity and not sess.busy:
            return sess.reset()
        if sess is not None and sess.busy:                      # an unfinished generator still owns it: leave it alone
            return DecodeSession(self.model, 1, capacity, use_graph, low_footprint=self.low_footprint)
        self._session, self._session_key = DecodeSession(self.model, 1, capacity, use_graph, low_footprint=self.low_footprint), key
        return self._session

    # -- scoring (the reference's forward(labels=...) / examples/evaluations/ppl.py on the session path) ------------------
    @torch.no_grad()
    def score_ids(self, sequences, labels=None, chunk: Optional[int] = None, head_rows: Optional[int] = None,
                  pad_id: int = 0, use_graph: Optional[bool] = None, reference_labels: bool = False):
        """Per-token log-probabilities of a batch of token-id sequences of any lengths: they are LEFT padded with ``pad_id``
        (the reference tokenizer's padding side), scored by ``DecodeSession.score`` on a session of that batch size (kept and
        reused like the generation session) and cut back to their own lengths.  ``labels``: one list per sequence, aligned with
        its ids, -100 = not scored (a prompt span); default: every token after a sequence's first is scored.
        ``reference_labels=True`` scores the first token of every PADDED sequence as well, from the pad in front of it - what the
        reference tokenizer's ``return_labels`` (chatglm_q/tokenizer.py:138-142: the ids, -100 at pads) makes its ``forward`` do, so
        that the loss is the reference's number for the batch; that entry is no function of the sequence (a pad's attention row is
        masked everywhere: it averages every key of the pass, so it moves with the batch's width and with ``chunk``) and is not
        part of the returned lists.  Returns
        ``(logprobs, loss)``: ``logprobs[b][t]`` = log p(sequences[b][t + 1] | sequences[b][:t + 1]) (``len - 1`` floats, 0.0 at
        unscored labels) and ``loss`` = minus the mean over every scored token of the batch, the reference's ``forward(labels=)``
        loss (chatglm_q/model.py:384-390)."""
        seqs = [list(map(int, s)) for s in sequences]
        if not seqs or any(len(s) == 0 for s in seqs):
            raise ValueError("score_ids: at least one sequence, none of them empty")
        if labels is not None:
            labels = [list(map(int, l)) for l in labels]
            if len(labels) != len(seqs) or any(len(l) != len(s) for l, s in zip(labels, seqs)):
                raise ValueError("score_ids: labels must match the sequences one to one, length by length")
        B, S = len(seqs), max(len(s) for s in seqs)
        limit = min(self.max_sequence_length, self.model.config.max_sequence_length)
        if S > limit:
            raise ValueError(f"score_ids: a sequence of {S} tokens exceeds the maximum sequence length {limit}")
        ids = torch.full((B, S), int(pad_id), dtype=torch.long)
        attn = torch.zeros(B, S, dtype=torch.long)
        lab = torch.full((B, S), -100, dtype=torch.long)
        for b, s in enumerate(seqs):
            ids[b, S - len(s):] = torch.tensor(s, dtype=torch.long)
            attn[b, S - len(s):] = 1
            lab[b, S - len(s):] = torch.tensor(labels[b] if labels is not None else s, dtype=torch.long)
            if not reference_labels:
                lab[b, S - len(s)] = -100                       # nothing in front of a sequence's first token but padding
        capacity = min(-(-S // 64) * 64, self.model.config.max_sequence_length)
        sess = self._session_for(capacity, use_graph, batch=B)
        sess.busy = True
        try:
            res = sess.score(ids, attention_mask=attn, labels=lab, chunk=chunk, head_rows=head_rows)
            rows = res.logprobs.cpu()                           # the call's one wait for the device
            loss = float(res.loss)
        finally:
            sess.busy = False
        return [rows[b, S - len(s):].tolist() for b, s in enumerate(seqs)], loss

    def perplexity(self, batches, **kw) -> float:
        """``exp(mean of the per-batch losses)`` over an iterable of batches (each a list of token-id sequences, scored by
        ``score_ids``) - the definition of the reference's perplexity run (examples/evaluations/ppl.py:31-45: batches of 20
        left-padded texts, ``loss, _, _ = model(**inputs)``, ``exp(sum(losses) / len(losses))``): a mean of batch means, not a mean
        over all tokens."""
        import math
        losses = [self.score_ids(batch, **kw)[1] for batch in batches]
        if not losses:
            raise ValueError("perplexity: no batches")
        return math.exp(sum(losses) / len(losses))

    def score(self, texts, **kw):
        """Text interface of ``score_ids`` when a tokenizer (``encode``) was supplied: one text or a list of texts."""
        if self.tokenizer is None:
            raise RuntimeError("no tokenizer: use score_ids() with token ids")
        single = isinstance(texts, str)
        logprobs, loss = self.score_ids([self.tokenizer.encode(t) for t in ([texts] if single else texts)], **kw)
        return (logprobs[0] if single else logprobs), loss

    @torch.no_grad()
    def generate_ids(self, prefix_ids: Iterable[int], max_generated_tokens: int = 400, top_k: int = 100,
                     top_p: float = 0.8, temperature: float = 1.0, greedy: bool = False, ignore_eos: bool = False,
                     prefill_chunk: Optional[int] = None, use_graph: Optional[bool] = None, sync_every_token: bool = True,
                     seed: Optional[int] = None, device_sampler: Optional[bool] = None, repetition_penalty: float = 1.0,
                     presence_penalty: float = 0.0, frequency_penalty: float = 0.0, logit_bias: Optional[dict] = None,
                     logprobs: Optional[int] = None, no_repeat_ngram_size: int = 0, bad_words_ids=None, stop_sequences=None,
                     min_new_tokens: int = 0, grammar=None):
        """Yields generated token ids one by one (batch 1, like the reference, chatglm_q/decoder.py:70).

        Default = the reference's only mode: top-k / top-p sampling (top_k 100, top_p 0.8, temperature 1.0).  On a GPU the
        sampler is one launch inside the captured step (``device_sampler`` None / True; False: the composed torch ops of
        ``top_p_sampling`` on the host's side of the loop, as the reference runs them) and draws from a counter-based generator
        seeded by ``seed`` (None: a seed taken from torch's global generator, so ``torch.manual_seed`` makes a run repeatable as it
        does for the reference's ``torch.multinomial``).  ``greedy=True``: argmax instead.

        Sampling controls (defaults: off, the path above exactly): ``repetition_penalty`` r > 0 divides the positive and
        multiplies the other logits of every id in the prompt or generated so far (the Hugging Face rule); ``presence_penalty`` p
        and ``frequency_penalty`` f subtract p + f x (times generated) from the logit of every id generated so far (OpenAI's
        rule); ``logit_bias`` ``{id: value}`` (at most ``fused_ops.LOGIT_BIAS_MAX`` entries, values finite or -inf: -inf bans the
        id) is added last.  They run as one more launch inside the captured step, in front of the argmax / the sampler, on the
        history kept on the device; ``last_stats["penalties"]`` says whether they were active.

        ``logprobs`` (None: off, the path above exactly): an int n in [0, ``fused_ops.TOP_LOGPROBS_MAX``] records every generated
        token's log-probability and the n most likely ids of its step with theirs - under the logits the selection read, after the
        sampling controls, before temperature / top-k / top-p - by one more launch behind the selection inside the captured step.
        The ids are yielded as before; when the generation ends (or the generator is closed) ``last_logprobs`` holds a
        ``GenerationLogprobs`` with one entry per token yielded, read from the device once; ``last_stats["logprobs"]`` says whether
        the record was on.

        History constraints (defaults: off, the path above exactly): ``no_repeat_ngram_size`` n >= 1 lets no n-gram of prompt +
        output occur twice (the Hugging Face rule; at most ``fused_ops.CONSTRAINT_SEQ_LEN_MAX``); ``bad_words_ids``, a list of id
        lists, bans each list's last id while the ids in front of it are the latest ones (a list of one id is banned always; the
        prompt counts); ``min_new_tokens`` keeps the end token out of the first that many tokens (nothing to do with
        ``ignore_eos`` or no end token); ``stop_sequences``, a list of id lists, ends the generation once the OUTPUT ends with one
        of them - the sequence is yielded, then the generator ends, as with the end token.  At most
        ``fused_ops.CONSTRAINT_SEQS_MAX`` sequences of all kinds together, each of at most ``CONSTRAINT_SEQ_LEN_MAX`` ids.  The bans
        run as one more launch inside the captured step, behind the penalties' and in front of the selection, on the ordered history
        kept on the device; stop sequences are matched by the host against the ids it reads anyway.  ``last_stats["constraints"]``
        says whether any of them was on, ``last_stats["stop_sequence"]`` which stop sequence the output ends with (None: none).

        ``grammar`` (None: off, the path above exactly): a ``grammar.ByteDFA`` or a pattern string (``grammar.compile_regex`` lists the
        syntax) the OUTPUT must match, at the byte level: after every token the concatenation of the generated ids' byte strings
        (``grammar.TokenBytes.join``; the end token excluded) is a viable prefix of the pattern's language, and the end token can be
        chosen only when it is a full match.  One more launch inside the captured step, behind the history constraints' and in front of
        the selection, on the automaton state kept on the device.  It needs an end token id (not ``ignore_eos``) and the vocabulary's
        byte table (``token_bytes=`` of the constructor, or a tokenizer with a sentencepiece file), and it does not go together with
        ``min_new_tokens``: the two can leave a row with nothing allowed.  (sentencepiece's ``decode`` drops one leading space of the
        joined bytes - its dummy prefix.)  ``last_stats["grammar"]`` says whether it was on, ``last_stats["grammar_state"]`` how the
        output ended: "accepted" (the end token, a full match), "open" (the budget ran out inside the pattern) or None.
        A ``grammar.BytePDA`` - ``grammar.json_grammar()``: JSON with arbitrary nesting - is taken wherever a ``ByteDFA`` is, under the
        same preconditions: the step then issues the pushdown automaton's launch (``fused_ops.pda_mask``) in the grammar launch's place,
        still exactly one launch more than an unconstrained step."""
        n_lp = check_logprobs(logprobs)
        self.last_logprobs = None
        prefix = list(prefix_ids)
        from . import fused_ops
        eos = None if ignore_eos or self.eos_token_id is None else int(self.eos_token_id)
        # (validated once, up front, all kinds together; the device is armed without the stop sequences: here the host matches them)
        (n_gram, min_new, table), = fused_ops.ConstraintState.check(1, no_repeat_ngram_size, bad_words_ids, stop_sequences, min_new_tokens,
                                                                    eos, vocab=self.model.config.vocab_size)
        stops = [q for kind, q in table if kind == fused_ops.ConstraintState.STOP]
        con_settings = [(n_gram, min_new, [e for e in table if e[0] != fused_ops.ConstraintState.STOP])]
        dfa = tokens = None
        if grammar is not None:
            from .grammar import as_grammar
            dfa = as_grammar(grammar)
            if eos is None:
                raise ValueError("grammar needs an end token id (eos_token_id, and not ignore_eos): the end token is how a match ends")
            if min_new > 0:
                raise ValueError("grammar and min_new_tokens do not go together: the two can leave a row with nothing allowed")
            tokens = self._grammar_table()
        limit = min(self.max_sequence_length, self.model.config.max_sequence_length)   # the cache cannot outgrow the rotary table
        budget = min(max_generated_tokens, limit - len(prefix))
        if budget <= 0:
            if n_lp is not None:
                self.last_logprobs = GenerationLogprobs([], [], [])
            return
        capacity = min(-(-(len(prefix) + budget) // 64) * 64, self.model.config.max_sequence_length)
        sess = self._session_for(capacity, use_graph)
        sess.busy = True
        try:
            pen = sess.arm_penalties([prefix], repetition_penalty, presence_penalty, frequency_penalty, logit_bias)
            con = sess.arm_constraints([prefix], checked=con_settings)
            gr = dfa is not None and sess.arm_grammar([dfa], eos, tokens)
            dev_sample = (not greedy) and sess.device_sampler_serves(top_k) and device_sampler is not False
            if device_sampler and not greedy and not dev_sample:
                raise ValueError(f"device_sampler=True needs a GPU and top_k <= 1024 (got {sess.device}, top_k {top_k})")
            if dev_sample:
                if seed is None:
                    seed = int(torch.randint(0, 2 ** 62, (1,)).item())
                sess.set_sampling(top_k, top_p, temperature, seed)
            # the keywords of every capture / decode_step of this generation
            step = dict(greedy=greedy, sample=dev_sample, pen=pen, lp=sess.arm_logprobs(n_lp is not None), con=con, **sess.grammar_stage(gr))
            inner = self._generate(sess, prefix, budget, top_k, top_p, temperature, ignore_eos, prefill_chunk, sync_every_token, step,
                                   stops, dfa)
            if n_lp is None:
                yield from inner
            else:
                returned = 0
                try:
                    for token in inner:
                        returned += 1
                        yield token
                finally:
                    inner.close()
                    # one read at the end, cut to the tokens handed out (the ahead-launch records one step past an end token)
                    self.last_logprobs = GenerationLogprobs(*sess.lp.read(0, n_lp, limit=returned))
        finally:
            sess.busy = False
            if POST_GENERATE_CHECK is not None:                 # set by chatglm_q_amd.dev.experiments: error words of one-launch MLPs
                POST_GENERATE_CHECK(sess)

    def _generate(self, sess: DecodeSession, prefix, budget: int, top_k: int, top_p: float, temperature: float, ignore_eos: bool,
                  prefill_chunk: Optional[int], sync_every_token: bool, step: dict, stops=(), dfa=None):
        # ``step``: the keywords of this generation's capture / decode_step calls; its plan says what runs around them
        plan = step_plan(**step)
        greedy, dev_sample, lp = step["greedy"], step["sample"], plan.lp
        # `auto`: the device picks the next token inside the step (argmax or the one-launch sampler) and feeds it back itself
        auto = plan.selector != "logits"
        times = []
        sync = (lambda: torch.cuda.synchronize(sess.device)) if sess.device.type == "cuda" else (lambda: None)

        t0 = time.perf_counter()
        logits = sess.first_logits(plan, sess.prefill(torch.tensor([prefix], dtype=torch.long), prefill_chunk))
        if dev_sample:
            nxt = sess.sample_first(logits)
        else:
            nxt = logits.argmax(-1) if greedy else top_p_sampling(logits, top_k, top_p, temperature)
            if lp:
                sess.tok.copy_(nxt.view(-1, 1))                    # the record reads the chosen id from device memory
        if lp:
            sess.logprobs_first(logits)
        token = int(nxt.item())                                    # the sync that makes the timing valid
        times.append(time.perf_counter() - t0)
        generated = [token]
        yield token

        # a stop sequence ends the generation as the end token does: matched against the ids the host reads anyway, yielded, then the end
        stopped = (lambda: matched_stop_sequence(generated, stops) is not None) if stops else (lambda: False)
        # (with stop sequences the host has to see every token: no loop in which it reads nothing until the end)
        device_loop = auto and not sync_every_token and (ignore_eos or self.eos_token_id is None) and not stops
        if len(generated) < budget and (ignore_eos or token != self.eos_token_id) and not stopped():
            sess.tok.fill_(token)
            sess.capture(**step)
        pending = []
        # Greedy or device-sampled decoding on a captured step: the graph feeds its own choice back, so step k + 1 does not wait for the HOST to have seen
        # token k.  It is launched before token k is read (one step of speculation: wasted - and harmless, the next prefill re-arms the
        # session - when token k turns out to be the end token), so the device never idles for the host's read-back + launch latency
        # (~20 us of a 1.15 ms token).  Tokens are yielded one by one as before.
        ahead = (auto and not device_loop and sess.graph is not None and sess.device.type == "cuda" and AHEAD_LAUNCH
                 and len(generated) < budget and (ignore_eos or token != self.eos_token_id) and not stopped())
        if ahead:
            ring = torch.empty((2, 1), dtype=torch.long).pin_memory()
            events = [torch.cuda.Event(), torch.cuda.Event()]

            def launch(k):
                sess.decode_step(None, **step)
                ring[k & 1].copy_(sess.tok.view(-1), non_blocking=True)
                events[k & 1].record()

            t0 = time.perf_counter()
            k = 0
            launch(0)
            while True:
                more = len(generated) + 1 < budget and sess.length + 1 <= sess.capacity     # a token after this one is wanted (and fits)
                if more:
                    launch(k + 1)
                events[k & 1].synchronize()
                token = int(ring[k & 1, 0])
                now = time.perf_counter()
                times.append(now - t0)
                t0 = now
                generated.append(token)
                yield token
                if not more or (not ignore_eos and token == self.eos_token_id) or stopped():
                    break
                k += 1
        while not ahead and len(generated) < budget and (ignore_eos or generated[-1] != self.eos_token_id) and not stopped():
            t0 = time.perf_counter()
            if device_loop:
                # the graph feeds its own choice back as the next input: the host only replays
                sess.decode_step(**step)
                pending.append(sess.tok.clone())
                generated.append(-1)
                times.append(time.perf_counter() - t0)
                continue
            logits = sess.decode_step(None if auto else torch.tensor([[generated[-1]]]), **step)
            if auto:
                nxt = sess.tok[:, 0]
            else:                                                  # the host samples: it adjusts, constrains and masks the logits it got back,
                logits = sess.host_logits(plan, logits)            # draws from them and records its own choice on them
                nxt = top_p_sampling(logits, top_k, top_p, temperature)
                if lp:
                    from . import fused_ops
                    fused_ops.step_logprobs(logits, nxt.view(-1).contiguous(), sess.lp)
            token = int(nxt.item())
            times.append(time.perf_counter() - t0)
            generated.append(token)
            yield token
        if device_loop and pending:
            t0 = time.perf_counter()
            sync()
            times[-1] += time.perf_counter() - t0
            toks = [int(t.item()) for t in pending]
            generated[-len(toks):] = toks
            for t in toks:
                yield t

        n = len(times)
        rest = sum(times[1:])
        grammar = "gr" in plan.stages or "pda" in plan.stages
        self.last_stats = {
            "prefix": len(prefix), "generated": n, "init_s": times[0], "sum_s": sum(times),
            "gen_tok_per_s": (n - 1) / rest if n > 1 and rest > 0 else float("nan"),
            "avg_tok_per_s": n / sum(times), "penalties": "pen" in plan.stages, "logprobs": lp,
            "constraints": "con" in plan.stages or bool(stops), "stop_sequence": matched_stop_sequence(generated, stops),
            "grammar": grammar, "grammar_state": self._grammar_result(dfa, generated, self.eos_token_id) if grammar else None,
        }
        if self.time_log:
            s = self.last_stats
            print("Decoder:")
            print(f"  len: {s['prefix']}(prefix) + {s['generated']}(gen)")
            print(f" init: {s['init_s']:.6f} s")
            print(f"  sum: {s['sum_s']:.6f} s")
            print(f"  gen: {s['gen_tok_per_s']:.6f} tok/s")
            print(f"  avg: {s['avg_tok_per_s']:.6f} tok/s")

    def generate(self, prefix_text: str, **kw):
        """Text interface when a tokenizer (``encode`` / ``decode``) was supplied; yields the decoded text so far."""
        if self.tokenizer is None:
            raise RuntimeError("no tokenizer: use generate_ids() with token ids")
        ids = []
        for tok in self.generate_ids(self.tokenizer.encode(prefix_text), **kw):
            ids.append(tok)
            yield self.tokenizer.decode(ids)

    # -- batched generation --------------------------------------------------------------------------------------------------------
    # Steps replayed between two looks at the live-row count.  The look is a non-blocking copy of 4 + 8 x batch bytes into pinned memory
    # and an event behind it; the host waits on the PREVIOUS group's event while the device runs the current group, so it never
    # idles the device, and a finished batch runs at most 2 x BATCH_POLL_EVERY + 1 steps past its last row's end.  Measured
    # (profiles/batch_generate_ab.txt): at 4 the whole loop runs at 0.995 - 1.000 of the raw greedy replay loop at batch 8 / 32, so
    # a larger group has nothing to win; an EOS run wasted 6 steps.
    BATCH_POLL_EVERY = 4
    SEED_STRIDE = 0x9E3779B97F4A7C15                            # seed=int: row b's seed is (seed + b * SEED_STRIDE) mod 2^63

    def _replay_polled(self, sess: DecodeSession, step: dict, max_steps: int, poll: int, live: Tensor, extra: Optional[Tensor] = None) -> int:
        """Capture the step ``step`` (the keywords of ``capture`` / ``decode_step``) and run it up to ``max_steps`` times, in groups of
        ``poll`` between two looks at the count in ``live`` (one int32: rows / prompts still running; ``extra``: a tensor copied to
        the host beside it); returns the steps run."""
        sess.capture(**step)
        cuda = sess.device.type == "cuda"
        if cuda:
            ring = torch.zeros((2, 1 + (extra.numel() if extra is not None else 0)), dtype=torch.int32).pin_memory()
            events = [torch.cuda.Event(), torch.cuda.Event()]
        steps = g = 0
        while steps < max_steps:
            n = min(poll, max_steps - steps)
            for _ in range(n):
                sess.decode_step(**step)
            steps += n
            if not cuda:
                if int(live[0]) == 0:
                    break
                continue
            ring[g & 1, :1].copy_(live, non_blocking=True)
            if extra is not None:
                ring[g & 1, 1:].copy_(extra.view(-1), non_blocking=True)
            events[g & 1].record()
            # the previous group's count: its event is behind the group the device is running now
            if g > 0:
                events[(g - 1) & 1].synchronize()
                if int(ring[(g - 1) & 1, 0]) == 0:
                    break
            g += 1
        return steps

    @torch.no_grad()
    def generate_batch_ids(self, prompts, max_generated_tokens=400, top_k=100, top_p=0.8, temperature=1.0, greedy=False,
                           seed=None, ignore_eos: bool = False, prefill_chunk: Optional[int] = None, use_graph: Optional[bool] = None,
                           poll_every: Optional[int] = None, repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0,
                           logit_bias=None, logprobs: Optional[int] = None, no_repeat_ngram_size=0, bad_words_ids=None,
                           stop_sequences=None, min_new_tokens=0, grammar=None):
        """Generate for a batch of prompts (lists of token ids, any lengths: LEFT padded with 0 as ``score_ids`` pads them) in one
        decode batch; returns one list of generated ids per prompt.  A row that stopped on the end token ends with it, as
        ``generate_ids`` yields it.

        ``max_generated_tokens``, ``top_k``, ``top_p``, ``temperature`` and ``greedy`` are scalars or one value per prompt; a
        greedy row is a top_k 1 row.  Defaults are the reference's sampler (chatglm_q/decoder.py:12-27), as in ``generate_ids``.
        ``seed``: one per prompt (row b's generator key is ``seed[b]``), an int (row 0 gets it, row b ``(seed + b *
        SEED_STRIDE) mod 2^63``) or None (the seeds come from torch's global generator: ``torch.manual_seed`` makes a run
        repeatable).  On a GPU every row draws from its own counter-based generator inside the captured step, so a row's tokens
        do not depend on its batch position, and a batch of one draws what ``generate_ids`` draws with the same seed.

        Budgets: row b may generate ``min(max_generated_tokens[b], limit - S)`` tokens, S = the longest prompt, limit = the maximum
        sequence length: the rows share one cache write index, so no row can run past the longest prompt's limit.  A row with
        budget 0 returns [].  Rows stop on the end token (unless ``ignore_eos``) or their budget; finished rows keep riding along
        (their compute is not skipped) until every row is done.  ``poll_every``: steps replayed between two looks at the live-row
        count (default BATCH_POLL_EVERY).

        ``repetition_penalty``, ``presence_penalty``, ``frequency_penalty`` and ``logit_bias`` (a dict ``{id: value}`` or None) are
        ``generate_ids``' sampling controls, each a scalar / one dict or one per prompt.  A row's history is its own prompt (the pads
        in front of it are no prompt tokens) and its own tokens; the controls run as one more launch in the captured step, so a
        row's tokens still do not depend on its batch position or on its neighbours' settings.  Defaults: off, the path above
        exactly; ``last_stats["penalties"]`` says whether they were active.

        ``logprobs`` (None: off) is ``generate_ids``' as well: with an int n in [0, ``fused_ops.TOP_LOGPROBS_MAX``] the step records
        every row's token log-prob and n alternatives on the device (finished rows record nothing), and ``last_logprobs`` holds one
        ``GenerationLogprobs`` per prompt, in prompt order, each as long as the row's returned ids.

        ``no_repeat_ngram_size``, ``bad_words_ids``, ``stop_sequences`` and ``min_new_tokens`` are ``generate_ids``' history constraints,
        each one value or one per prompt; for the two sequence arguments the nesting depth decides - a list of id lists applies to every
        row, a list of one such list (or None) per prompt gives every row its own.  They run as one more launch in the captured step on
        every row's own ordered history.  A row that has generated one of its stop sequences is finished ON THE DEVICE by the step
        that follows (one row-step is spent on seeing it) and its ids end with the sequence.  Defaults: off, the path above exactly;
        ``last_stats["constraints"]`` says whether they were active, ``last_stats["stop_sequence"]`` holds, per row, which of its stop
        sequences its ids end with (None: none).

        ``grammar`` is ``generate_ids``' too: one ``grammar.ByteDFA`` / pattern string for every row, or a list with one per prompt, None
        for an unconstrained row - every row follows its own automaton in the same launch, and a row without one gets the ids of the
        same call without ``grammar``.  A row with a grammar needs the end token and must not have ``min_new_tokens``.
        ``last_stats["grammar"]`` says whether any row had one, ``last_stats["grammar_state"]`` holds "accepted" / "open" / None per row."""
        n_lp = check_logprobs(logprobs)
        self.last_logprobs = None
        prompts = [list(map(int, p)) for p in prompts]
        if not prompts or any(len(p) == 0 for p in prompts):
            raise ValueError("generate_batch_ids: at least one prompt, none of them empty")
        B = len(prompts)
        from . import fused_ops

        def per_row(name, v, conv):
            return [conv(x) for x in fused_ops.per_row(name, v, B, "generate_batch_ids", "prompts")]

        wanted = per_row("max_generated_tokens", max_generated_tokens, int)
        ks, ps = per_row("top_k", top_k, int), per_row("top_p", top_p, float)
        ts, gr = per_row("temperature", temperature, float), per_row("greedy", greedy, bool)
        if any(not t > 0 for t in ts):
            raise ValueError("generate_batch_ids: temperature > 0")
        if any(k < 1 for k in ks):
            raise ValueError("generate_batch_ids: top_k >= 1")
        ks = [1 if g else k for g, k in zip(gr, ks)]
        on_gpu = self.model.final_ln.weight.device.type == "cuda"
        if on_gpu and any(k > fused_ops.SAMPLER_MAX_TOP_K for k in ks) and self.model.config.vocab_size > fused_ops.SAMPLER_MAX_TOP_K:
            raise ValueError(f"generate_batch_ids: top_k <= {fused_ops.SAMPLER_MAX_TOP_K} on a GPU (got {max(ks)})")
        if seed is None:
            seeds = torch.randint(0, 2 ** 62, (B,)).tolist()
        elif isinstance(seed, (list, tuple)):
            seeds = per_row("seed", seed, int)
        else:
            seeds = [(int(seed) + b * self.SEED_STRIDE) & 0x7FFFFFFFFFFFFFFF for b in range(B)]
        poll = self.BATCH_POLL_EVERY if poll_every is None else int(poll_every)
        if poll < 1:
            raise ValueError("generate_batch_ids: poll_every >= 1")
        S = max(len(p) for p in prompts)
        limit = min(self.max_sequence_length, self.model.config.max_sequence_length)
        budgets = [max(0, min(w, limit - S)) for w in wanted]
        # (validated up front: wrong lengths / values raise before anything runs)
        pen_args = (per_row("repetition_penalty", repetition_penalty, float), per_row("presence_penalty", presence_penalty, float),
                    per_row("frequency_penalty", frequency_penalty, float), per_row("logit_bias", logit_bias, lambda d: d))
        fused_ops.PenaltyState.check(B, self.model.config.vocab_size, list(zip(*pen_args[:3])), pen_args[3])
        stop = None if ignore_eos or self.eos_token_id is None else int(self.eos_token_id)
        con_settings = fused_ops.ConstraintState.check(B, no_repeat_ngram_size, bad_words_ids, stop_sequences, min_new_tokens, stop,
                                                       vocab=self.model.config.vocab_size)
        row_stops = [[q for kind, q in table if kind == fused_ops.ConstraintState.STOP] for _, _, table in con_settings]
        dfas, tokens = [None] * B, None
        if grammar is not None:
            from .grammar import as_grammar
            compiled = {}                                       # (a pattern given for every row is compiled once)
            for b, g in enumerate(fused_ops.ConstraintState.per_row("grammar", grammar, B)):
                if g is not None:
                    dfas[b] = compiled[id(g)] if id(g) in compiled else compiled.setdefault(id(g), as_grammar(g))
            for b in range(B):
                if dfas[b] is not None and stop is None:
                    raise ValueError("grammar needs an end token id (eos_token_id, and not ignore_eos): the end token is how a match ends")
                if dfas[b] is not None and con_settings[b][1] > 0:
                    raise ValueError(f"row {b}: grammar and min_new_tokens do not go together: the two can leave a row with nothing allowed")
            if any(d is not None for d in dfas):
                tokens = self._grammar_table()
        if max(budgets) == 0:
            self.last_stats = {"batch": B, "prefix": [len(p) for p in prompts], "generated": [0] * B, "steps": 0, "penalties": False,
                               "logprobs": n_lp is not None, "constraints": False, "stop_sequence": [None] * B,
                               "grammar": False, "grammar_state": [None] * B}
            if n_lp is not None:
                self.last_logprobs = [GenerationLogprobs([], [], []) for _ in prompts]
            return [[] for _ in prompts]
        ids = torch.zeros((B, S), dtype=torch.long)
        attn = torch.zeros((B, S), dtype=torch.long)
        for b, p in enumerate(prompts):
            ids[b, S - len(p):] = torch.tensor(p, dtype=torch.long)
            attn[b, S - len(p):] = 1
        capacity = min(-(-(S + max(budgets)) // 64) * 64, self.model.config.max_sequence_length)
        sess = self._session_for(capacity, use_graph, batch=B)
        sess.busy = True
        try:
            sess.arm_rows(list(zip(ks, ps, ts)), seeds, budgets, stop)
            pen = sess.arm_penalties(prompts, *pen_args)
            con = sess.arm_constraints(prompts, checked=con_settings)
            gr = tokens is not None and sess.arm_grammar(dfas, stop, tokens)
            lp = sess.arm_logprobs(n_lp is not None)
            step = dict(greedy=False, rows=True, pen=pen, lp=lp, con=con, **sess.grammar_stage(gr))
            t0 = time.perf_counter()
            logits = sess.first_logits(step_plan(**step), sess.prefill(ids, prefill_chunk, attention_mask=attn))
            sess.sample_rows_first(logits)
            if lp:
                sess.logprobs_first(logits, rows=True)
            live = int(sess.rows.live.item())                   # the sync that makes the first-token time valid
            t_first = time.perf_counter() - t0
            steps, max_steps = 0, max(budgets) - 1
            if live > 0 and max_steps > 0:
                steps = self._replay_polled(sess, step, max_steps, poll, sess.rows.live, sess.rows.row_state)
            out = sess.rows.out_tokens.cpu()                    # one copy of the tokens at the end
            state = sess.rows.row_state.cpu()
            total = time.perf_counter() - t0
            record = sess.lp.fetch() if lp else None            # ... and one of every buffer of the log-prob record
        finally:
            sess.busy = False
        counts = [int(state[b, 0]) for b in range(B)]
        res = [out[b, :counts[b]].tolist() for b in range(B)]
        if lp:
            self.last_logprobs = [GenerationLogprobs(*sess.lp.read(b, n_lp, limit=counts[b], host=record)) for b in range(B)]
        gen = sum(counts)
        rest = total - t_first
        self.last_stats = {
            "batch": B, "prefix": [len(p) for p in prompts], "generated": counts, "steps": steps,
            "invalid": [b for b in range(B) if int(state[b, 1]) & fused_ops.BatchRows.INVALID],
            "prefill_s": t_first, "sum_s": total,
            "gen_tok_per_s": (gen - sum(1 for c in counts if c)) / rest if steps and rest > 0 else float("nan"),
            "avg_tok_per_s": gen / total if total > 0 else float("nan"), "penalties": bool(pen), "logprobs": bool(lp),
            "constraints": bool(con), "stop_sequence": [matched_stop_sequence(res[b], row_stops[b]) for b in range(B)],
            "grammar": bool(gr), "grammar_state": [self._grammar_result(dfas[b], res[b], stop) for b in range(B)],
        }
        if self.time_log:
            s = self.last_stats
            print("Decoder (batch):")
            print(f"  len: {B} rows, {max(s['prefix'])}(longest prefix) + {s['generated']}(gen), {s['steps']} steps")
            print(f" init: {s['prefill_s']:.6f} s")
            print(f"  sum: {s['sum_s']:.6f} s")
            print(f"  gen: {s['gen_tok_per_s']:.6f} tok/s")
            print(f"  avg: {s['avg_tok_per_s']:.6f} tok/s")
        return res

    @torch.no_grad()
    def beam_search_ids(self, prompts, num_beams: int = 4, max_generated_tokens: int = 400, length_penalty: float = 1.0,
                        early_stopping: bool = True, num_return_sequences: int = 1, ignore_eos: bool = False,
                        prefill_chunk: Optional[int] = None, use_graph: Optional[bool] = None, poll_every: Optional[int] = None):
        """Beam search for one prompt (a list of token ids) or a list of prompts (any lengths: LEFT padded with 0) in one decode batch of
        ``len(prompts) * num_beams`` rows; returns, per prompt, a list of at most ``num_return_sequences`` ``BeamHypothesis(ids, score,
        sum_logprob)``, the best first (for a single id list: that prompt's list).

        Every step runs on the device inside the captured decode step - the rows' ``2 * num_beams`` best ids (``step_logprobs``' walk),
        the cross-beam selection with its finished-hypothesis heap (``qlinear_beam_advance``) and the reorder of the key/value cache by
        parent beam, in place (``qlinear_beam_gather``): three launches behind the model's.  The host replays the step in groups of
        ``poll_every`` (default BATCH_POLL_EVERY) and looks at the count of prompts still searching, as ``generate_batch_ids`` does; the
        sequences are never copied on the device - a (token, parent) trellis is read once at the end and walked backwards.

        The rules (tests/_beam_oracle.py): a hypothesis' score is ``sum_logprob / length ** length_penalty``; an end token among a
        prompt's ``num_beams`` best candidates finishes a hypothesis; ``early_stopping=True`` ends a prompt's search once ``num_beams``
        hypotheses are finished, ``False`` once additionally none of the running beams can beat the worst of them at the current
        length.  A prompt still searching when the budget ``min(max_generated_tokens, limit - S)`` runs out (S = the longest prompt,
        limit = the maximum sequence length) adds its running beams as hypotheses.  A budget of 0 returns ``[]`` per prompt.  With
        ``ignore_eos`` (or no end token) nothing finishes early.  ``num_beams=1`` is greedy decoding.  Sampling, penalties, logit bias,
        log-prob records, history constraints and grammars are not part of a beam search."""
        from . import fused_ops
        single = len(prompts) > 0 and not isinstance(prompts[0], (list, tuple))
        prompts = [list(map(int, p)) for p in ([prompts] if single else prompts)]
        if not prompts or any(len(p) == 0 for p in prompts):
            raise ValueError("beam_search_ids: at least one prompt, none of them empty")
        if isinstance(num_beams, bool) or not isinstance(num_beams, int) or not 1 <= num_beams <= fused_ops.BEAMS_MAX:
            raise ValueError(f"beam_search_ids: num_beams must be an int in [1, {fused_ops.BEAMS_MAX}] (got {num_beams!r})")
        if isinstance(num_return_sequences, bool) or not isinstance(num_return_sequences, int) or not 1 <= num_return_sequences <= num_beams:
            raise ValueError(f"beam_search_ids: num_return_sequences must be an int in [1, num_beams] (got {num_return_sequences!r})")
        vocab = self.model.config.vocab_size
        if vocab < 2 * num_beams:
            raise ValueError(f"beam_search_ids: a vocabulary of {vocab} supplies no {2 * num_beams} candidates per beam")
        fused_ops.beam_norm_table(1, length_penalty)            # (validates the penalty)
        poll = self.BATCH_POLL_EVERY if poll_every is None else int(poll_every)
        if poll < 1:
            raise ValueError("beam_search_ids: poll_every >= 1")
        P, B = len(prompts), num_beams
        R = P * B
        S = max(len(p) for p in prompts)
        limit = min(self.max_sequence_length, self.model.config.max_sequence_length)
        if S > limit:
            raise ValueError(f"beam_search_ids: a prompt of {S} tokens exceeds the maximum sequence length {limit}")
        budget = max(0, min(int(max_generated_tokens), limit - S))
        eos = None if ignore_eos or self.eos_token_id is None else int(self.eos_token_id)
        if budget == 0:
            self.last_stats = {"prompts": P, "beams": B, "prefix": [len(p) for p in prompts], "steps": 0}
            return [] if single else [[] for _ in prompts]
        ids = torch.zeros((R, S), dtype=torch.long)
        attn = torch.zeros((R, S), dtype=torch.long)
        for g, p in enumerate(prompts):
            ids[g * B:(g + 1) * B, S - len(p):] = torch.tensor(p, dtype=torch.long)
            attn[g * B:(g + 1) * B, S - len(p):] = 1
        capacity = min(-(-(S + budget) // 64) * 64, self.model.config.max_sequence_length)
        sess = self._session_for(capacity, use_graph, batch=R) if R != 1 else self._session_for(capacity, use_graph)
        sess.busy = True
        try:
            st = sess.arm_beams(B, eos, length_penalty, early_stopping, first=S)
            t0 = time.perf_counter()
            logits = sess.prefill(ids, prefill_chunk, attention_mask=attn)
            sess.beam_first(logits)
            live = int(st.live.item())                          # the sync that makes the first-token time valid
            t_first = time.perf_counter() - t0
            steps, max_steps = 0, budget - 1
            if live > 0 and max_steps > 0:
                steps = self._replay_polled(sess, dict(greedy=False, beam=True), max_steps, poll, st.live)
            host = st.fetch()                                   # one copy of every buffer at the end
            norm = st.norm.cpu()
            total = time.perf_counter() - t0
        finally:
            sess.busy = False
        res = self._beam_results(host, norm, P, B, eos, num_return_sequences)
        rest = total - t_first
        self.last_stats = {
            "prompts": P, "beams": B, "prefix": [len(p) for p in prompts], "steps": steps,
            "searched": [int(host["steps"][g]) for g in range(P)], "done": [bool(int(host["done"][g])) for g in range(P)],
            "prefill_s": t_first, "sum_s": total, "steps_per_s": steps / rest if steps and rest > 0 else float("nan"),
        }
        if self.time_log:
            s = self.last_stats
            print("Decoder (beam search):")
            print(f"  len: {P} prompts x {B} beams, {max(s['prefix'])}(longest prefix), {s['steps']} steps")
            print(f" init: {s['prefill_s']:.6f} s")
            print(f"  sum: {s['sum_s']:.6f} s")
            print(f"  gen: {s['steps_per_s']:.6f} steps/s")
        return res[0] if single else res

    @staticmethod
    def _beam_results(host, norm, P: int, B: int, eos, n_return: int):
        """The budget end on the host: a group that is not done adds its running beams under the heap rule; per prompt the hypotheses
        are sorted by score descending, then earlier finish step, then lower slot, and walked back through the trellis."""
        trellis = host["trellis"]

        def backtrack(row, slots):
            ids = []
            for s in range(slots - 1, -1, -1):
                tok, row = int(trellis[s, row, 0]), int(trellis[s, row, 1])
                ids.append(tok)
            return ids[::-1]

        out = []
        for g in range(P):
            r0, cnt, t = g * B, int(host["fin_count"][g]), int(host["steps"][g])
            heap = [(host["fin_score"][r0 + s], int(host["fin_len"][r0 + s]), int(host["fin_row"][r0 + s]), host["fin_sum"][r0 + s], True)
                    for s in range(cnt)]
            if not int(host["done"][g]) and t > 0:
                for r in range(r0, r0 + B):
                    entry = (host["beam_score"][r] / norm[t], t, r, host["beam_score"][r], False)     # one fp32 division
                    if len(heap) < B:
                        heap.append(entry)
                        continue
                    worst = 0
                    for s in range(1, B):
                        if bool(heap[s][0] <= heap[worst][0]):
                            worst = s
                    if bool(entry[0] > heap[worst][0]):
                        heap[worst] = entry
            key = [float("-inf") if bool(torch.isnan(e[0])) else float(e[0]) for e in heap]
            order = sorted(range(len(heap)), key=lambda s: (-key[s], heap[s][1], s))
            hyps = []
            for s in order[:n_return]:
                score, n, row, total, ended = heap[s]
                ids = backtrack(row, n - 1) + [int(eos)] if ended else backtrack(row, n)
                hyps.append(BeamHypothesis(ids, float(score), float(total)))
            out.append(hyps)
        return out

    def beam_search(self, texts, **kw):
        """Text interface of ``beam_search_ids`` when a tokenizer (``encode`` / ``decode``) was supplied: per prompt a list of
        ``(text, score)``, the best first (for a single string: that prompt's list)."""
        if self.tokenizer is None:
            raise RuntimeError("no tokenizer: use beam_search_ids() with token ids")
        single = isinstance(texts, str)
        outs = self.beam_search_ids([self.tokenizer.encode(t) for t in ([texts] if single else texts)], **kw)
        res = [[(self.tokenizer.decode(h.ids), h.score) for h in hyps] for hyps in outs]
        return res[0] if single else res

    def generate_batch(self, prefix_texts, **kw):
        """Text interface of ``generate_batch_ids`` when a tokenizer (``encode`` / ``decode``) was supplied: one decoded text per
        prompt."""
        if self.tokenizer is None:
            raise RuntimeError("no tokenizer: use generate_batch_ids() with token ids")
        outs = self.generate_batch_ids([self.tokenizer.encode(t) for t in prefix_texts], **kw)
        return [self.tokenizer.decode(o) for o in outs]

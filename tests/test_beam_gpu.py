"""Beam search on the GPU: the candidates against ``step_logprobs``, ``qlinear_beam_advance`` against the Python oracle
(tests/_beam_oracle.py) as bit patterns, ``qlinear_beam_gather`` against ``index_select`` on clones with sentinel margins, and
``ChatGLMDecoder.beam_search_ids`` against the test's own loop (eager "logits" steps, the oracle, ``index_select`` on the cache)."""
import numpy as np
import pytest
import torch

import _beam_cases as BC
import _beam_oracle as BO
from chatglm_q_amd import _lib, fused_ops
from chatglm_q_amd.decoder import ChatGLMDecoder, DecodeSession
from test_model_cpu import build as build_tiny

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TDT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}


# ---- candidates ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("B", [1, 4, 10])
def test_candidates_are_step_logprobs(dt, B):
    R, W = 2 * B, 2 * B
    g = torch.Generator().manual_seed(B)
    for N in (W, 251, 65024):
        x = (torch.randn(R, N, generator=g) * 3).to(TDT[dt])
        x[0, : min(N, 6)] = x[0, 0]                              # a tie group at the front of one row
        x = x.to(DEV)
        tok = torch.zeros(R, dtype=torch.int64, device=DEV)
        st = fused_ops.BeamState(R, 4, DEV).arm(2, B)
        ref = fused_ops.StepLogprobs(R, 3, DEV, n_top=W)
        fused_ops.step_logprobs(x, tok, st.cand)
        fused_ops.step_logprobs(x, tok, ref)
        assert st.cand.count.tolist() == [1] * R
        assert torch.equal(st.cand.top_ids[:, 0], ref.top_ids[:, 0])
        assert np.array_equal(BC.bits(st.cand.top_lp[:, 0]), BC.bits(ref.top_lp[:, 0]))
        order = torch.sort(x.float(), dim=-1, descending=True, stable=True)[1][:, :W]
        assert torch.equal(st.cand.top_ids[:, 0].long(), order)
        # the advance frees the one-slot record: the next step's candidates land in slot 0 again
        fused_ops.beam_advance(st, tok)
        assert st.cand.count.tolist() == [0] * R
        fused_ops.step_logprobs(x.flip(0).contiguous(), tok, st.cand)
        assert st.cand.count.tolist() == [1] * R and torch.equal(st.cand.top_ids[:, 0], ref.top_ids[:, 0].flip(0))


# ---- the advance against the oracle -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,B,length_penalty,early", BC.CONFIGS)
def test_advance_equals_oracle(P, B, length_penalty, early):
    """The scenarios test_beam_cpu.py proves to meet every case of the rules (ties across rows, the end id in front of and behind rank
    B, a full heap that replaces and one that does not, done beside live groups, -inf initial scores, the trellis' first and last slot
    and a full trellis), every buffer as bit patterns after every step, with and without the step's bookkeeping."""
    for seed in range(3):
        BC.run_scenario(DEV, P, B, 11, length_penalty, early, n_steps=10, cap=9, seed=seed, book=seed == 1)
    BC.run_scenario(DEV, P, B, None, length_penalty, early, n_steps=4, cap=9, seed=5, book=True, capacity=8)    # no end id; the mask's last column


def test_advance_argument_errors_return_status_codes():
    lib = _lib.get_lib()
    st = fused_ops.BeamState(4, 8, DEV).arm(2, 2)
    tok = torch.zeros(4, dtype=torch.int64, device=DEV)
    c = st.cand

    def call(P=2, B=2, cap=8, tok_ptr=tok.data_ptr(), wi=None, pos=None, mask=None):
        return lib.qlinear_beam_advance(P, B, c.top_ids.data_ptr(), c.top_lp.data_ptr(), c.count.data_ptr(), st.beam_score.data_ptr(), tok_ptr,
                                        st.parent.data_ptr(), st.trellis.data_ptr(), cap, st.steps.data_ptr(), st.fin_score.data_ptr(),
                                        st.fin_sum.data_ptr(), st.fin_len.data_ptr(), st.fin_row.data_ptr(), st.fin_count.data_ptr(),
                                        st.done.data_ptr(), st.live.data_ptr(), st.norm.data_ptr(), st.cfg.data_ptr(), wi, pos, mask, 16, None)

    before = _lib.launch_count()
    assert call(B=0) != 0 and call(B=11) != 0 and call(cap=0) != 0 and call(tok_ptr=None) != 0
    assert call(wi=tok.data_ptr()) != 0                          # an incomplete bookkeeping triple
    assert call(P=0) == 0 and _lib.launch_count() == before
    table = torch.zeros(1, dtype=torch.int64, device=DEV)
    first, end = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
    gather = lambda **kw: lib.qlinear_beam_gather(*[kw.get(k, d) for k, d in (("table", table.data_ptr()), ("n", 1), ("P", 2), ("B", 2), ("cap", 8),
                                                                              ("pb", 32), ("parent", st.parent.data_ptr()),
                                                                              ("first", first.data_ptr()), ("end", end.data_ptr()))], None)
    assert gather(B=11) != 0 and gather(pb=3) != 0 and gather(cap=0) != 0 and gather(parent=None) != 0
    assert gather(n=0) == 0 and _lib.launch_count() == before
    torch.cuda.synchronize()


# ---- the gather ---------------------------------------------------------------------------------------------------------------------
KINDS = ["identity", "first", "cycle", "dup", "outside"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("P,B", [(1, 2), (2, 4), (1, 10), (2, 3)])
def test_gather_equals_index_select(kind, P, B):
    w = 41
    for tail, dtype in (((2, 128), torch.float16), ((2, 32), torch.float16)):                # 512 B: ChatGLM2's; 128 B: the tiny model's
        for first, end in ((0, w), (w - 1, w), (w, w), (5, 64), (7, 100)):                   # whole, one position, empty, to / past the capacity
            BC.run_gather(DEV, P, B, 64, tail, dtype, kind, first, end)
    for tail, dtype in (((2, 3), torch.float16), ((1, 3), torch.float16), ((3,), torch.float32)):   # 12 B, 6 B, 12 B: the narrow chunks
        BC.run_gather(DEV, P, B, 64, tail, dtype, kind, 3, w)
    torch.cuda.synchronize()


@pytest.mark.parametrize("kind", ["cycle", "dup"])
def test_gather_at_capacity_2048(kind):
    BC.run_gather(DEV, 2, 4, 2048, (2, 128), torch.float16, kind, 100, 2001)
    BC.run_gather(DEV, 1, 10, 2048, (2, 128), torch.float16, kind, 0, 2048)
    torch.cuda.synchronize()


# ---- end to end on the tiny model ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny16():
    return build_tiny("f16", DEV)


P1, P2, T = [17, 3, 99, 250, 8, 61], [44, 3], 12


def loop_beams(model, prompts, B, T, eos, length_penalty, early, n_return):
    """The test's own loop: an eager "logits" session over P x B rows, the prefix broadcast by ``index_select``, ``step_logprobs`` for
    the rows' candidates, the Python oracle for the merge - with an explicit id list per beam, no trellis - and ``index_select`` on the
    cache by parent.  Returns per prompt [(ids, score, sum_logprob)]."""
    P, S = len(prompts), max(len(p) for p in prompts)
    R = P * B
    ids = torch.zeros((R, S), dtype=torch.long)
    attn = torch.zeros((R, S), dtype=torch.long)
    for g, p in enumerate(prompts):
        ids[g * B:(g + 1) * B, S - len(p):] = torch.tensor(p)
        attn[g * B:(g + 1) * B, S - len(p):] = 1
    sess = DecodeSession(model, R, 64, use_graph=False)
    logits = sess.prefill(ids.to(DEV), attention_mask=attn.to(DEV))
    lead = torch.arange(R, device=DEV) // B * B
    for buf in sess.cache.k + sess.cache.v:
        buf[:, :S] = buf.index_select(0, lead)[:, :S]
    oracle = BO.Beams(P, B, eos, length_penalty, early, 64)
    rec = fused_ops.StepLogprobs(R, 1, DEV, n_top=2 * B)
    seqs = [[] for _ in range(R)]
    ended = {}                                                   # (group, heap slot) -> ids of the hypothesis that sits there
    for t in range(1, T + 1):
        rec.arm()
        fused_ops.step_logprobs(logits, sess.tok.view(-1), rec)
        tok, parent = oracle.advance(rec.top_ids[:, 0].cpu().tolist(), [[np.float32(v) for v in row] for row in rec.top_lp[:, 0].cpu().numpy()])
        for g in range(P):
            for slot, e in enumerate(oracle.heap[g]):
                if e[1] == t and oracle.steps[g] == t:
                    ended[(g, slot)] = seqs[e[2]] + [eos]
        seqs = [seqs[parent[r]] + [tok[r]] if oracle.steps[r // B] == t else seqs[r] for r in range(R)]
        if t == T:
            break
        order = torch.tensor(parent, device=DEV)
        for buf in sess.cache.k + sess.cache.v:
            buf.copy_(buf.index_select(0, order))
        logits = sess.decode_step(torch.tensor(tok, dtype=torch.long, device=DEV)[:, None], greedy=False)
    out = []
    for g in range(P):
        heap = [(e[0], e[1], ended[(g, slot)], e[3]) for slot, e in enumerate(oracle.heap[g])]
        if not oracle.done[g]:
            n = oracle.steps[g]
            for r in range(g * B, g * B + B):
                BO.heap_add(heap, B, (BO.fdiv(oracle.score[r], oracle.norm[n]), n, seqs[r], oracle.score[r]))
        order = sorted(range(len(heap)), key=lambda s: (-float(BO.order_key(heap[s][0])), heap[s][1], s))
        out.append([(heap[s][2], float(heap[s][0]), float(heap[s][3])) for s in order[:n_return]])
    return out


def as_tuples(res):
    return [[(h.ids, h.score, h.sum_logprob) for h in hyps] for hyps in res]


@pytest.mark.parametrize("B", [1, 3, 4])
@pytest.mark.parametrize("prompts", [[P1], [P1, P2]], ids=["one", "two"])
def test_beam_search_equals_the_loop(prompts, B, tiny16):
    model, cfg = tiny16
    greedy = list(ChatGLMDecoder(cfg, model).generate_ids(P1, max_generated_tokens=T, greedy=True, ignore_eos=True))
    for eos, length_penalty, early in ((None, 1.0, True), (greedy[2], 1.0, True), (greedy[2], 2.5, False), (greedy[1], 0.0, False)):
        dec = ChatGLMDecoder(cfg, model, eos_token_id=eos)
        kw = dict(num_beams=B, max_generated_tokens=T, length_penalty=length_penalty, early_stopping=early, num_return_sequences=B)
        got = as_tuples(dec.beam_search_ids(prompts, use_graph=True, **kw))
        sess = dec._batch_sessions[len(prompts) * B][1] if len(prompts) * B > 1 else dec._session
        assert "beam" in sess._graphs                            # the steps were replays of the captured step
        want = loop_beams(model, prompts, B, T, eos, length_penalty, early, B)
        assert got == want                                       # identical ids, bit-identical scores
        assert got == as_tuples(dec.beam_search_ids(prompts, use_graph=False, **kw))
        if eos is not None and B == 1 and early:                 # one beam is the greedy run: it ends on the id that run emits early
            assert got[0][0][0] == greedy[:greedy.index(eos) + 1] and dec.last_stats["done"][0]


def test_one_beam_is_greedy(tiny16):
    model, cfg = tiny16
    dec = ChatGLMDecoder(cfg, model)
    greedy = list(dec.generate_ids(P1, max_generated_tokens=T, greedy=True, ignore_eos=True))
    assert dec.beam_search_ids(P1, num_beams=1, max_generated_tokens=T, ignore_eos=True)[0].ids == greedy
    dec = ChatGLMDecoder(cfg, model, eos_token_id=greedy[3])
    assert dec.beam_search_ids(P1, num_beams=1, max_generated_tokens=T)[0].ids == list(dec.generate_ids(P1, max_generated_tokens=T, greedy=True))


def test_session_reuse(tiny16):
    model, cfg = tiny16
    dec = ChatGLMDecoder(cfg, model)
    kw = dict(max_generated_tokens=T, greedy=True, ignore_eos=True)
    fresh = ChatGLMDecoder(cfg, model).generate_batch_ids([P1, P2, P1, P2], **kw)
    first = as_tuples(dec.beam_search_ids([P1], num_beams=4, max_generated_tokens=T, ignore_eos=True, num_return_sequences=4))
    sess = dec._batch_sessions[4][1]
    graph = sess._graphs["beam"]
    # a greedy generation on the same session (batch 4) after the search: what a fresh decoder returns
    assert dec.generate_batch_ids([P1, P2, P1, P2], **kw) == fresh
    assert "beam" in sess._graphs and "rows" in sess._graphs and dec._batch_sessions[4][1] is sess
    # another prompt length: the captured step serves it
    other = as_tuples(dec.beam_search_ids([P2], num_beams=4, max_generated_tokens=T, ignore_eos=True, num_return_sequences=4))
    assert sess._graphs["beam"] is graph
    assert other == loop_beams(model, [P2], 4, T, None, 1.0, True, 4)
    assert as_tuples(dec.beam_search_ids([P1], num_beams=4, max_generated_tokens=T, ignore_eos=True, num_return_sequences=4)) == first
    assert sess._graphs["beam"] is graph
    # another beam count on the same rows: the step is captured again, the results are the loop's
    two = as_tuples(dec.beam_search_ids([P1, P2], num_beams=2, max_generated_tokens=T, ignore_eos=True, num_return_sequences=2))
    assert two == loop_beams(model, [P1, P2], 2, T, None, 1.0, True, 2) and sess._graphs["beam"] is not graph
    # batch 1: "beam" beside "greedy"
    one = ChatGLMDecoder(cfg, model)
    g1 = list(one.generate_ids(P1, **kw))
    one.beam_search_ids(P1, num_beams=1, max_generated_tokens=T, ignore_eos=True)
    assert "beam" in one._session._graphs and "greedy" in one._session._graphs
    assert list(one.generate_ids(P1, **kw)) == g1


def test_launch_accounting(tiny16):
    model, cfg = tiny16
    B, S = 4, len(P1)
    ids = torch.tensor([P1] * B, device=DEV)
    sess = DecodeSession(model, B, 64, use_graph=False)
    sess.arm_beams(B, None, 1.0, True, first=S)
    sess.beam_first(sess.prefill(ids))
    sess.decode_step(greedy=False, beam=True)                    # (lazy layouts exist now)
    before = _lib.launch_count()
    sess.decode_step(greedy=False, beam=True)
    beam = _lib.launch_count() - before
    plain = DecodeSession(model, B, 64, use_graph=False)
    plain.prefill(ids)
    tok = torch.zeros(B, 1, dtype=torch.long, device=DEV)
    plain.decode_step(tok, greedy=False)
    before = _lib.launch_count()
    plain.decode_step(tok, greedy=False)
    assert beam == _lib.launch_count() - before + 3
    assert plain.beams is None                                   # a session that never beams holds nothing extra

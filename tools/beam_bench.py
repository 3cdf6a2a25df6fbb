"""Developer tool: what beam search inside the decode step costs (profiles/beam_search_ab.txt).

1. Each of a beam step's three launches alone under graph replay, one prompt x B = 4 and 10 beams: the candidates
   (``qlinear_step_logprobs``, fp16 logits (B, 65024), 2B alternatives), ``qlinear_beam_advance`` and ``qlinear_beam_gather`` over the 56
   cache buffers of ChatGLM2-6B ((B, 8192, 2, 128) fp16) at generated lengths 32 / 1 024 / 8 000 behind a 32-id prompt - the gather
   with identity parents (the group exits behind the parent loads) and with a full permutation (every row moves).  Candidates and
   advance do not depend on the generated length.  A graph of ``--chain`` launches is replayed; per launch: the median over the
   replays / chain.  Yardsticks, measured the same way in the same run: the empty launch (probe kernel of libqlinear_hip_span.so,
   csrc/probe_kernels.hip) and a plain device copy (``Tensor.copy_``) of the bytes the permuted gather moves.
2. Steps per second after the first token on the synthetic 28-layer ChatGLM2-6B int4g32 model (``bench_extras._chatglm2_6b``): a
   4-beam search (``beam_search_ids``) against batched greedy decoding at batch 4 (``generate_batch_ids``) with the same 32-id prompt
   and ``--tokens`` tokens, EOS ignored, the two legs ALTERNATED round by round in one process after an untimed warm-up of each; per
   leg the median of the rounds and their [min .. max].

    python tools/beam_bench.py [--rounds 5] [--tokens 128] [--skip-model] [--out profiles/beam_search_ab.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

import bench_extras  # noqa: E402
from chatglm_q_amd import _lib, fused_ops  # noqa: E402
from chatglm_q_amd.decoder import ChatGLMDecoder  # noqa: E402
from logprobs_bench import REPS, V, dev, probe_lib, replay_us  # noqa: E402

LENGTHS = (32, 1024, 8000)
PROMPT, CAPACITY, LAYERS, POS = 32, 8192, 28, (2, 128)


def launches_alone(chain, say):
    probes = probe_lib()
    g = torch.Generator().manual_seed(3)
    records = 1 + chain * (REPS + 4) + 8                         # every launch of a chain appends one entry
    fmt = lambda r: f"{r[0]:7.2f} [{r[1]:.2f} .. {r[2]:.2f}]"
    say(f"1. the three launches of a beam step alone, graph of {chain} launches replayed {REPS} times, us per launch: median [min .. max]")
    say(f"   one prompt x B beams; candidates: fp16 logits (B, {V}), 2B alternatives; gather: {2 * LAYERS} buffers (B, {CAPACITY}, 2, 128) fp16,")
    say(f"   positions [{PROMPT}, {PROMPT} + L); copy: Tensor.copy_ of the bytes the permuted gather reads (it writes as many)")
    empty = replay_us(lambda: probes.qlinear_probe_empty(256, _lib.stream_ptr(dev)), chain)
    say(f"   empty launch {fmt(empty)}")
    for B in (4, 10):
        lg = (torch.randn(B, V, generator=g) * 3).half().to(dev)
        tok = torch.zeros(B, dtype=torch.int64, device=dev)
        rec = fused_ops.StepLogprobs(B, records, dev, n_top=2 * B)
        cand = replay_us(lambda: fused_ops.step_logprobs(lg, tok, rec), chain)
        st = fused_ops.BeamState(B, records, dev).arm(1, B, None, 1.0, True, first=PROMPT)
        fused_ops.step_logprobs(lg, tok, st.cand)
        adv = replay_us(lambda: fused_ops.beam_advance(st, tok), chain)
        assert int(st.steps[0]) > chain and int(st.live[0]) == 1
        say(f"   B {B:2d}: candidates {fmt(cand)}   advance {fmt(adv)}")
        bufs = [torch.zeros((B, CAPACITY) + POS, dtype=torch.float16, device=dev) for _ in range(2 * LAYERS)]
        table = fused_ops.BeamGatherTable(bufs)
        first = torch.tensor([PROMPT], dtype=torch.int32, device=dev)
        ident = torch.arange(B, dtype=torch.int32, device=dev)
        perm = ((torch.arange(B) + 1) % B).to(torch.int32).to(dev)
        for L in LENGTHS:
            end = torch.tensor([PROMPT + L], dtype=torch.int64, device=dev)
            nbytes = 2 * LAYERS * B * L * POS[0] * POS[1] * 2
            src, dst = (torch.zeros(nbytes, dtype=torch.uint8, device=dev) for _ in range(2))
            res = {"identity": replay_us(lambda: fused_ops.beam_gather(table, ident, first, end, B), chain),
                   "permuted": replay_us(lambda: fused_ops.beam_gather(table, perm, first, end, B), chain),
                   "copy": replay_us(lambda: dst.copy_(src), chain)}
            say(f"         L {L:5d} ({nbytes / 2 ** 20:7.1f} MiB): gather identity {fmt(res['identity'])}   permuted {fmt(res['permuted'])}   "
                f"copy {fmt(res['copy'])}   permuted / copy {res['permuted'][0] / res['copy'][0]:.2f}   identity / empty {res['identity'][0] / empty[0]:.2f}")
            del src, dst
        del bufs, table


def model_legs(rounds, T, say):
    model, cfg = bench_extras._chatglm2_6b(torch, dev, torch.float16)
    for mod in model.modules():
        if hasattr(mod, "prepare"):
            mod.prepare()
    dec = ChatGLMDecoder(None, model)
    prompt = [(37 * i + 11) % cfg.vocab_size for i in range(32)]

    def beam():
        out = dec.beam_search_ids(prompt, num_beams=4, max_generated_tokens=T, ignore_eos=True)
        assert len(out[0].ids) == T and dec.last_stats["steps"] == T - 1
        return dec.last_stats["steps_per_s"]

    def greedy():
        out = dec.generate_batch_ids([prompt] * 4, greedy=True, max_generated_tokens=T, ignore_eos=True)
        assert [len(o) for o in out] == [T] * 4
        return dec.last_stats["gen_tok_per_s"] / 4               # every step yields one token per row

    legs = {"greedy batch 4": greedy, "4 beams": beam}
    for fn in legs.values():                                     # untimed warm-up: layouts, graphs, allocator
        fn()
    res = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            res[k].append(fn())
    say(f"2. synthetic ChatGLM2-6B int4g32, one 32-id prompt, {T} tokens, EOS ignored, decode steps per second after the first token, "
        f"{rounds} alternated rounds: median [min .. max]")
    med = {k: statistics.median(v) for k, v in res.items()}
    for k, v in res.items():
        say(f"   {k:15s}: {med[k]:8.1f} [{min(v):.1f} .. {max(v):.1f}] steps/s   ({1e6 / med[k]:.1f} us per step)")
    say(f"   4 beams / greedy batch 4 = {med['4 beams'] / med['greedy batch 4']:.4f}   (+{1e6 / med['4 beams'] - 1e6 / med['greedy batch 4']:.1f} us per step)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--tokens", type=int, default=128)
    ap.add_argument("--chain", type=int, default=64)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"tools/beam_bench.py on {torch.cuda.get_device_name(0)}")
    launches_alone(a.chain, say)
    if not a.skip_model:
        model_legs(a.rounds, a.tokens, say)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

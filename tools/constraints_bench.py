"""Developer tool: what the history constraints (``no_repeat_ngram_size`` / ``bad_words_ids`` / ``stop_sequences`` / ``min_new_tokens``:
``qlinear_history_constraints``) cost (profiles/generation_constraints_ab.txt).

1. The launch alone under graph replay: fp16 logits, N = 65024, batch 1 / 8 / 32, n = 3 and no sequences, at history lengths 32 /
   1 024 / 8 128.  The history buffer is exactly as long as the history, so every launch of the chain reads ``tok``, finds the history
   full, appends nothing and scans the same L positions.  Histories: ids drawn from the whole vocabulary (the window's first compare
   rejects almost every position: a handful of stores), and at 8 128 also ids from a 5-id alphabet (about one position in 25 matches:
   hundreds of stores, all to 5 addresses).  A graph of ``--chain`` launches is replayed; per launch: the median over the replays /
   chain.  Next to it, measured the same way in the same run, the yardsticks: the empty launch (probe kernel of
   libqlinear_hip_span.so, csrc/probe_kernels.hip) and ``qlinear_logit_penalties`` on the same logits.
2. Generated tokens per second after the first token on the synthetic 28-layer ChatGLM2-6B int4g32 model
   (``bench_extras._chatglm2_6b``), 32-id prompts, ``--tokens`` tokens, EOS ignored: greedy and sampled, batch 1 (``generate_ids``)
   / 8 / 32 (``generate_batch_ids``), the controls off against on (no_repeat_ngram_size 3 and two banned sequences), the legs
   ALTERNATED round by round in one process after an untimed warm-up of each; per leg the median of the rounds and their
   [min .. max]; then on / off next to the ratio the launch time of part 1 predicts, step / (step + launch).

    python tools/constraints_bench.py [--rounds 5] [--tokens 128] [--skip-model] [--out profiles/generation_constraints_ab.txt]

The off path needs no timing: with every control at its default it issues and replays exactly the launches it did before the controls
existed (tests/test_constraints_gpu.py::test_launch_accounting).
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

LENGTHS = (32, 1024, 8128)
ON = dict(no_repeat_ngram_size=3, bad_words_ids=[[11, 12], [13]])


def constraint_state(B, L, alphabet, g):
    st = fused_ops.ConstraintState(B, L, dev)
    hist = torch.randint(0, alphabet, (B, L), generator=g).tolist()
    st.arm(hist, fused_ops.ConstraintState.check(B, no_repeat_ngram_size=3))
    st.prompt_len.fill_(32)
    return st


def launch_alone(chain, say):
    probes = probe_lib()
    g = torch.Generator().manual_seed(3)
    out = {}
    say(f"1. qlinear_history_constraints alone, graph of {chain} launches replayed {REPS} times, us per launch: median [min .. max]")
    say(f"   fp16 logits (B, {V}), n = 3, no sequences, the history full at L ids (every launch scans L positions, appends nothing);")
    say("   ids from the whole vocabulary, '5 ids': from a 5-id alphabet; yardsticks measured the same way in the same run")
    for B in (1, 8, 32):
        lg = (torch.randn(B, V, generator=g) * 3).half().to(dev)
        tok = torch.randint(0, V, (B,), generator=g).to(dev)
        states = {(L, "vocab"): constraint_state(B, L, V, g) for L in LENGTHS}
        states[(LENGTHS[-1], "5 ids")] = constraint_state(B, LENGTHS[-1], 5, g)
        pen = fused_ops.PenaltyState(B, V, dev).arm([list(range(32))] * B, [(1.3, 0.5, 0.25)] * B, None)
        bodies = {k: (lambda st=st: fused_ops.history_constraints(lg, st, tok)) for k, st in states.items()}
        bodies["empty"] = lambda: probes.qlinear_probe_empty(256, _lib.stream_ptr(dev))
        bodies["penalties"] = lambda: fused_ops.logit_penalties(lg, pen, tok)
        res = {k: replay_us(fn, chain) for k, fn in bodies.items()}
        for (L, _), st in states.items():
            assert st.hist_len.tolist() == [L] * B, "a launch appended: the history was not full"
        out[B] = res[(1024, "vocab")][0]
        fmt = lambda k: f"{res[k][0]:6.2f} [{res[k][1]:.2f} .. {res[k][2]:.2f}]"
        say(f"   B {B:2d}: " + "   ".join(f"L {L} {fmt((L, 'vocab'))}" for L in LENGTHS) + f"   L {LENGTHS[-1]}, 5 ids {fmt((LENGTHS[-1], '5 ids'))}"
            f"   empty launch {fmt('empty')}   penalties {fmt('penalties')}")
        top = res[(LENGTHS[-1], "vocab")][0]
        say(f"         L {LENGTHS[-1]} / penalties {top / res['penalties'][0]:.2f}   L {LENGTHS[-1]} / empty {top / res['empty'][0]:.2f}   "
            f"L 32 / empty {res[(32, 'vocab')][0] / res['empty'][0]:.2f}")
    return out


def model_legs(rounds, T, launch_us, say):
    model, cfg = bench_extras._chatglm2_6b(torch, dev, torch.float16)
    for mod in model.modules():
        if hasattr(mod, "prepare"):
            mod.prepare()
    dec = ChatGLMDecoder(None, model)
    prompt = lambda b: [(37 * i + 11 + 101 * b) % cfg.vocab_size for i in range(32)]

    def leg(B, greedy, on):
        kw = ON if on else {}

        def run():
            if B == 1:
                out = [list(dec.generate_ids(prompt(0), greedy=greedy, seed=5, max_generated_tokens=T, ignore_eos=True, **kw))]
            else:
                out = dec.generate_batch_ids([prompt(b) for b in range(B)], greedy=greedy, seed=list(range(B)), max_generated_tokens=T,
                                             ignore_eos=True, **kw)
            assert [len(o) for o in out] == [T] * B and dec.last_stats["constraints"] is on
            return dec.last_stats["gen_tok_per_s"]
        return run

    legs = {(B, mode, on): leg(B, greedy, on) for B in (1, 8, 32) for mode, greedy in (("greedy", True), ("sampled", False))
            for on in (False, True)}
    for fn in legs.values():                                     # untimed warm-up: layouts, graphs, allocator
        fn()
    res = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            res[k].append(fn())
    med = {k: statistics.median(v) for k, v in res.items()}
    say(f"2. synthetic ChatGLM2-6B int4g32, 32-id prompts, {T} tokens, EOS ignored, generated tok/s after the first token (all rows), "
        f"{rounds} alternated rounds: median [min .. max]")
    say(f"   on = {ON}; on/off = tok/s with the controls over tok/s without; predicted = step / (step + L 1024 launch of part 1), "
        "step = B / (tok/s off)")
    for B in (1, 8, 32):
        for mode in ("greedy", "sampled"):
            off, on = med[(B, mode, False)], med[(B, mode, True)]
            step_us = B / off * 1e6
            pred = step_us / (step_us + launch_us[B]) if launch_us else float("nan")
            rng = lambda k: f"[{min(res[k]):.1f} .. {max(res[k]):.1f}]"
            say(f"   B {B:2d} {mode:7s}: off {off:8.1f} {rng((B, mode, False))}   on {on:8.1f} {rng((B, mode, True))} on/off {on / off:.4f} "
                f"(+{step_us * (off / on - 1):.2f} us)   predicted {pred:.4f} (step {step_us:.1f} us, +{launch_us.get(B, float('nan')):.2f} us)")


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
    say(f"tools/constraints_bench.py on {torch.cuda.get_device_name(0)}")
    launch_us = launch_alone(a.chain, say)
    if not a.skip_model:
        model_legs(a.rounds, a.tokens, launch_us, say)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

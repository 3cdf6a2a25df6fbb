"""Developer tool: what batched generation (``ChatGLMDecoder.generate_batch_ids``) costs against the parent code paths
(profiles/batch_generate_ab.txt).

On the synthetic 28-layer ChatGLM2-6B int4g32 model (``bench_extras._chatglm2_6b``), 32-id prompts, 128 generated tokens, EOS
ignored, aggregate generated tokens per second after the first token (the reference's ``gen`` definition summed over rows):
  * batch 8 / 32, greedy and sampled (reference defaults) ``generate_batch_ids`` against the raw batched greedy loop of
    ``bench_extras.e2e_generate`` ("batched_decode": capture the greedy step, replay it);
  * batch 1, greedy and sampled ``generate_batch_ids([p])`` against ``generate_ids(p)`` of the same mode.
The legs are ALTERNATED round by round in one process after an untimed warm-up of each; per leg the median of the rounds and
their [min .. max].  Then one EOS run at batch 8: steps replayed after the last row finished.

``--kernels`` instead launches the selection kernels alone (batch 1 / 8 / 32 x 65024 fp16 logits: batch_sample_advance greedy
and sampled, greedy_advance, top_p_sample), for a ``rocprofv3 --kernel-trace --stats`` run of their own:

    python tools/batch_generate_bench.py [--rounds 3] [--poll-every N]
    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/batch_generate_bench.py --kernels
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench_extras  # noqa: E402
from chatglm_q_amd import fused_ops  # noqa: E402
from chatglm_q_amd.decoder import ChatGLMDecoder, DecodeSession  # noqa: E402

dev = torch.device("cuda:0")
V = 65024


def kernels(reps=200):
    g = torch.Generator().manual_seed(3)
    for B in (1, 8, 32):
        lg = (torch.randn(B, V, generator=g) * 3).half().to(dev)
        tok = torch.zeros(B, dtype=torch.int64, device=dev)
        cap = 64
        widx = torch.zeros(1, dtype=torch.int64, device=dev)
        pos = torch.zeros(B, dtype=torch.int64, device=dev)
        mask = torch.zeros((B, 1, cap), dtype=torch.float32, device=dev)
        for label, k in (("greedy", 1), ("sampled", 100)):
            rows = fused_ops.BatchRows(B, reps, dev).arm([(k, 0.8, 1.0)] * B, list(range(B)), [reps] * B)
            for _ in range(reps):
                fused_ops.batch_sample_advance(lg, tok, rows, widx, pos, mask)
                widx.zero_()
        for _ in range(reps):
            fused_ops.greedy_advance(lg, tok[:, None], widx, pos[:, None], mask)
            widx.zero_()
        rng = fused_ops.new_rng_state(B, 1, dev)
        params = torch.tensor([100.0, 0.8, 1.0], device=dev)
        for _ in range(reps):
            fused_ops.top_p_sample(lg, tok, rng, dev_params=params, write_index=widx, pos=pos, mask=mask)
            widx.zero_()
    torch.cuda.synchronize()
    print("kernels launched: batch 1 / 8 / 32 x", V, "fp16 logits,", reps, "launches each")


def raw_greedy_loop(model, prompts, n_tokens):
    """The parent's batched greedy decode (bench_extras.e2e_generate "batched_decode"): prefill, argmax, capture, replay."""
    B = len(prompts)
    sb = DecodeSession(model, B, 256, use_graph=True)
    lg = sb.prefill(torch.tensor(prompts, device=dev))
    sb.tok.copy_(lg.argmax(-1, keepdim=True))
    sb.capture(greedy=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n_tokens - 1):
        sb.decode_step(greedy=True)
    torch.cuda.synchronize()
    return B * (n_tokens - 1) / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--tokens", type=int, default=128)
    ap.add_argument("--poll-every", type=int, default=None)
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args()
    if a.kernels:
        kernels()
        return
    model, cfg = bench_extras._chatglm2_6b(torch, dev, torch.float16)
    for mod in model.modules():
        if hasattr(mod, "prepare"):
            mod.prepare()
    dec = ChatGLMDecoder(None, model)
    T = a.tokens
    prompt = lambda b: [(37 * i + 11 + 101 * b) % cfg.vocab_size for i in range(32)]
    kw = dict(max_generated_tokens=T, ignore_eos=True, poll_every=a.poll_every)

    def batch_leg(B, greedy):
        def run():
            out = dec.generate_batch_ids([prompt(b) for b in range(B)], greedy=greedy, seed=list(range(B)), **kw)
            assert [len(o) for o in out] == [T] * B
            return dec.last_stats["gen_tok_per_s"]
        return run

    def one_leg(greedy):
        def run():
            out = list(dec.generate_ids(prompt(0), greedy=greedy, seed=5, max_generated_tokens=T, ignore_eos=True))
            assert len(out) == T
            return dec.last_stats["gen_tok_per_s"]
        return run

    legs = {}
    for B in (8, 32):
        legs[f"raw_greedy_loop_b{B}"] = (lambda B=B: raw_greedy_loop(model, [prompt(b) for b in range(B)], T))
        legs[f"batch_greedy_b{B}"] = batch_leg(B, True)
        legs[f"batch_sampled_b{B}"] = batch_leg(B, False)
    legs["generate_ids_greedy_b1"] = one_leg(True)
    legs["batch_greedy_b1"] = batch_leg(1, True)
    legs["generate_ids_sampled_b1"] = one_leg(False)
    legs["batch_sampled_b1"] = batch_leg(1, False)
    for fn in legs.values():                                    # untimed warm-up: layouts, graphs, allocator
        fn()
    res = {k: [] for k in legs}
    for r in range(a.rounds):
        for k, fn in legs.items():
            res[k].append(fn())
    med = {k: statistics.median(v) for k, v in res.items()}
    print(f"poll_every {a.poll_every or ChatGLMDecoder.BATCH_POLL_EVERY}, {T} tokens, 32-id prompts, {a.rounds} alternated rounds")
    for k, v in res.items():
        print(f"  {k:28s} {med[k]:9.1f} tok/s  [{min(v):.1f} .. {max(v):.1f}]")
    print("ratios against the parent-code yardsticks (bar 0.97):")
    for B in (8, 32):
        for m in ("greedy", "sampled"):
            print(f"  batch_{m}_b{B} / raw_greedy_loop_b{B}: {med[f'batch_{m}_b{B}'] / med[f'raw_greedy_loop_b{B}']:.4f}")
    for m in ("greedy", "sampled"):
        print(f"  batch_{m}_b1 / generate_ids_{m}_b1: {med[f'batch_{m}_b1'] / med[f'generate_ids_{m}_b1']:.4f}")
    # EOS: sampled rows (fixed seeds: the same streams with and without the end token); the end token is the one that every row
    # produces and whose latest first occurrence over the rows is the earliest from step 16 on; steps replayed after the last row finished
    prompts = [prompt(b) for b in range(8)]
    skw = dict(seed=list(range(8)), max_generated_tokens=T, poll_every=a.poll_every)
    base = dec.generate_batch_ids(prompts, ignore_eos=True, **skw)
    common = set(base[0]).intersection(*map(set, base[1:]))
    ends = {t: max(row.index(t) for row in base) for t in common}
    ends = {t: e for t, e in ends.items() if e >= 16}
    eos = min(ends, key=ends.get) if ends else base[0][40]
    dec_eos = ChatGLMDecoder(None, model, eos_token_id=eos)
    out = dec_eos.generate_batch_ids(prompts, **skw)
    last = max(len(o) for o in out) - 1
    print(f"EOS run (batch 8 sampled, end token {eos}): rows ended at {[len(o) for o in out]} tokens; last row finished at step {last}, "
          f"{dec_eos.last_stats['steps']} steps run, {dec_eos.last_stats['steps'] - last} wasted (bound: 2 x poll_every + 1)")


if __name__ == "__main__":
    main()

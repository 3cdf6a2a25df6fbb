"""Developer tool: what the sampling controls (repetition / presence / frequency penalties, logit bias:
``qlinear_logit_penalties``) cost (profiles/logit_penalties_ab.txt).

1. The launch alone under graph replay: fp16 logits, N = 65024, batch 1 / 8 / 32, a history of 32 prompt ids and 200 generated
   tokens per row, every rule on, 4 bias entries per row.  A graph of ``--chain`` launches is replayed; per launch: the median over
   the replays / chain.  Next to it, measured the same way with the probe kernels of libqlinear_hip_span.so
   (csrc/probe_kernels.hip): the empty launch, and the pure streaming read of the bytes the pass must move (B x N x (2 + 4):
   logits + state words).  Everything in the chain is cache-warm, as the logits are in a decode step (lm_head has just written
   them).
2. Generated tokens per second after the first token on the synthetic 28-layer ChatGLM2-6B int4g32 model
   (``bench_extras._chatglm2_6b``), 32-id prompts, ``--tokens`` tokens, EOS ignored: greedy and sampled, batch 1 (``generate_ids``)
   / 8 / 32 (``generate_batch_ids``), penalties on against off, the legs ALTERNATED round by round in one process after an untimed
   warm-up of each; per leg the median of the rounds and their [min .. max]; then on / off next to the ratio the launch time of
   part 1 predicts, (step + launch) / step.

    python tools/penalty_bench.py [--rounds 5] [--tokens 128] [--skip-model] [--out profiles/logit_penalties_ab.txt]

Penalties off against the parent commit is the whole-step A/B of tools/decode_ab.py (one process per tree, interleaved).
"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench_extras  # noqa: E402
from chatglm_q_amd import _lib, fused_ops  # noqa: E402
from chatglm_q_amd.decoder import ChatGLMDecoder  # noqa: E402

dev = torch.device("cuda:0")
V = 65024
PEN = dict(repetition_penalty=1.2, presence_penalty=0.3, frequency_penalty=0.1)


def probe_lib():
    path = os.path.join(ROOT, "chatglm_q_amd", "csrc", "libqlinear_hip_span.so")
    lib = ctypes.CDLL(path)
    lib.qlinear_probe_empty.argtypes = [ctypes.c_int, ctypes.c_void_p]
    lib.qlinear_probe_read.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
    lib.qlinear_probe_read_waves.restype = ctypes.c_int64
    lib.qlinear_probe_read_waves.argtypes = [ctypes.c_int64]
    return lib


def replay_us(body, chain, reps=30):
    """Median microseconds per launch of ``body`` captured ``chain`` times into one graph."""
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        body()
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(chain):
            body()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        graph.replay()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / chain)
    return statistics.median(times), min(times), max(times)


def launch_alone(chain, say):
    probes = probe_lib()
    g = torch.Generator().manual_seed(3)
    out = {}
    say(f"1. qlinear_logit_penalties alone, graph of {chain} launches replayed 30 times, us per launch: median [min .. max]")
    say(f"   fp16 logits (B, {V}); per row 32 prompt ids, 200 generated tokens, r/p/f = 1.2/0.3/0.1, 4 bias entries; bytes = B x N x (2 + 4)")
    for B in (1, 8, 32):
        lg = (torch.randn(B, V, generator=g) * 3).half().to(dev)
        prompts = [torch.randint(0, V, (32,), generator=g).tolist() for _ in range(B)]
        st = fused_ops.PenaltyState(B, V, dev).arm(prompts, [(1.2, 0.3, 0.1)] * B, [{7: -1.0, 900: float("-inf"), 40000: 2.0, 65023: 0.5}] * B)
        for _ in range(200):
            fused_ops.logit_penalties(lg, st, torch.randint(0, V, (B,), generator=g).to(dev))
        tok = torch.randint(0, V, (B,), generator=g).to(dev)
        nbytes = B * V * 6
        region = torch.zeros(nbytes // 4, dtype=torch.int32, device=dev)
        sink = torch.zeros(int(probes.qlinear_probe_read_waves(nbytes)) + 64, dtype=torch.int32, device=dev)

        def pen():                                               # in place on the same logits: the values drift, the traffic does not
            fused_ops.logit_penalties(lg, st, tok)

        def empty():
            probes.qlinear_probe_empty(256, _lib.stream_ptr(dev))

        def read():
            probes.qlinear_probe_read(region.data_ptr(), nbytes, sink.data_ptr(), _lib.stream_ptr(dev))
        res = {k: replay_us(fn, chain) for k, fn in (("penalties", pen), ("empty", empty), ("read", read))}
        out[B] = res["penalties"][0]
        say(f"   B {B:2d}: penalties {res['penalties'][0]:6.2f} [{res['penalties'][1]:.2f} .. {res['penalties'][2]:.2f}]   "
            f"empty launch {res['empty'][0]:5.2f} [{res['empty'][1]:.2f} .. {res['empty'][2]:.2f}]   "
            f"streaming read of {nbytes / 1e6:.2f} MB {res['read'][0]:5.2f} [{res['read'][1]:.2f} .. {res['read'][2]:.2f}]   "
            f"read / penalties {res['read'][0] / res['penalties'][0]:.2f}")
    return out


def model_legs(rounds, T, launch_us, say):
    model, cfg = bench_extras._chatglm2_6b(torch, dev, torch.float16)
    for mod in model.modules():
        if hasattr(mod, "prepare"):
            mod.prepare()
    dec = ChatGLMDecoder(None, model)
    prompt = lambda b: [(37 * i + 11 + 101 * b) % cfg.vocab_size for i in range(32)]
    bias = {5: float("-inf"), 77: -1.0}

    def leg(B, greedy, on):
        extra = dict(PEN, logit_bias=bias) if on else {}

        def run():
            if B == 1:
                out = [list(dec.generate_ids(prompt(0), greedy=greedy, seed=5, max_generated_tokens=T, ignore_eos=True, **extra))]
            else:
                out = dec.generate_batch_ids([prompt(b) for b in range(B)], greedy=greedy, seed=list(range(B)), max_generated_tokens=T,
                                             ignore_eos=True, **extra)
            assert [len(o) for o in out] == [T] * B and dec.last_stats["penalties"] is on
            return dec.last_stats["gen_tok_per_s"]
        return run

    legs = {}
    for B in (1, 8, 32):
        for mode, greedy in (("greedy", True), ("sampled", False)):
            for on in (False, True):
                legs[(B, mode, on)] = leg(B, greedy, on)
    for fn in legs.values():                                     # untimed warm-up: layouts, graphs, allocator
        fn()
    res = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            res[k].append(fn())
    med = {k: statistics.median(v) for k, v in res.items()}
    say(f"2. synthetic ChatGLM2-6B int4g32, 32-id prompts, {T} tokens, EOS ignored, generated tok/s after the first token (all rows), "
        f"{rounds} alternated rounds: median [min .. max]")
    say("   on/off = tok/s with penalties over tok/s without; predicted = step / (step + launch of part 1), step = B / (tok/s off)")
    for B in (1, 8, 32):
        for mode in ("greedy", "sampled"):
            off, on = med[(B, mode, False)], med[(B, mode, True)]
            step_us = B / off * 1e6
            pred = step_us / (step_us + launch_us[B]) if launch_us else float("nan")
            say(f"   B {B:2d} {mode:7s}: off {off:8.1f} [{min(res[(B, mode, False)]):.1f} .. {max(res[(B, mode, False)]):.1f}]   "
                f"on {on:8.1f} [{min(res[(B, mode, True)]):.1f} .. {max(res[(B, mode, True)]):.1f}]   on/off {on / off:.4f}   "
                f"predicted {pred:.4f}   (step {step_us:.1f} us, +{step_us * (off / on - 1):.2f} us measured, +{launch_us.get(B, float('nan')):.2f} us predicted)")


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
    say(f"tools/penalty_bench.py on {torch.cuda.get_device_name(0)}")
    launch_us = launch_alone(a.chain, say)
    if not a.skip_model:
        model_legs(a.rounds, a.tokens, launch_us, say)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

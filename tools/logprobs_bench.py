"""Developer tool: what per-token log-probabilities during generation (``logprobs=n``: ``qlinear_step_logprobs``) cost
(profiles/generation_logprobs_ab.txt).

1. The launch alone under graph replay: fp16 logits, N = 65024, batch 1 / 8 / 32, seeded normal rows at scale 3, with n_top = 0 (one
   walk) and n_top = 20 (two walks + the selection).  A graph of ``--chain`` launches is replayed; per launch: the median over the
   replays / chain.  Next to it, measured the same way in the same run, the yardsticks: the empty launch and the pure streaming
   read of the B x N x 2 bytes (probe kernels of libqlinear_hip_span.so, csrc/probe_kernels.hip), the arg-max launch
   (``qlinear_greedy_advance``) and the sampler launch (``qlinear_top_p_sample``, top_k 100 / top_p 0.8, with the bookkeeping).
   Everything in the chain is cache-warm, as the logits are in a decode step (lm_head has just written them, the selection has just
   read them).  The record is sized so that no launch of the run finds it full (checked at the end).
2. Generated tokens per second after the first token on the synthetic 28-layer ChatGLM2-6B int4g32 model
   (``bench_extras._chatglm2_6b``), 32-id prompts, ``--tokens`` tokens, EOS ignored: greedy and sampled, batch 1 (``generate_ids``)
   / 8 / 32 (``generate_batch_ids``), ``logprobs`` None against 0 and 5, the legs ALTERNATED round by round in one process after an
   untimed warm-up of each; per leg the median of the rounds and their [min .. max]; then on / off next to the ratio the launch time
   of part 1 predicts, step / (step + launch).  (The session's record is always QL_TOP_LOGPROBS_MAX wide - one captured graph serves
   every n - so 0 and 5 run the same launch; they differ in what the host reads at the end.)

    python tools/logprobs_bench.py [--rounds 5] [--tokens 128] [--skip-model] [--out profiles/generation_logprobs_ab.txt]

``logprobs=None`` against the parent commit is the whole-step A/B of tools/decode_ab.py (one process per tree, interleaved): the off
path issues and replays exactly the launches it did.
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
REPS = 30


def probe_lib():
    path = os.path.join(ROOT, "chatglm_q_amd", "csrc", "libqlinear_hip_span.so")
    lib = ctypes.CDLL(path)
    lib.qlinear_probe_empty.argtypes = [ctypes.c_int, ctypes.c_void_p]
    lib.qlinear_probe_read.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
    lib.qlinear_probe_read_waves.restype = ctypes.c_int64
    lib.qlinear_probe_read_waves.argtypes = [ctypes.c_int64]
    return lib


def replay_us(body, chain, reps=REPS):
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
    cap = chain * (REPS + 3) + 8                                 # every launch of a variant's run finds a free slot
    say(f"1. qlinear_step_logprobs alone, graph of {chain} launches replayed {REPS} times, us per launch: median [min .. max]")
    say(f"   fp16 logits (B, {V}), normal x 3; yardsticks measured the same way in the same run; bytes = B x N x 2")
    for B in (1, 8, 32):
        lg = (torch.randn(B, V, generator=g) * 3).half().to(dev)
        tok = torch.randint(0, V, (B,), generator=g).to(dev)
        states = {n: fused_ops.StepLogprobs(B, cap, dev, n_top=n) for n in (0, 20)}
        nbytes = B * V * 2
        region = torch.zeros(nbytes // 4, dtype=torch.int32, device=dev)
        sink = torch.zeros(int(probes.qlinear_probe_read_waves(nbytes)) + 64, dtype=torch.int32, device=dev)
        gtok = torch.zeros(B, 1, dtype=torch.int64, device=dev)
        wi = torch.zeros(1, dtype=torch.int64, device=dev)
        pos = torch.zeros(B, 1, dtype=torch.int64, device=dev)
        mask = torch.zeros(B, 1, 4096, dtype=torch.float32, device=dev)
        rng = fused_ops.new_rng_state(B, 5, dev)

        def lp0():
            fused_ops.step_logprobs(lg, tok, states[0])

        def lp20():
            fused_ops.step_logprobs(lg, tok, states[20])

        def empty():
            probes.qlinear_probe_empty(256, _lib.stream_ptr(dev))

        def read():
            probes.qlinear_probe_read(region.data_ptr(), nbytes, sink.data_ptr(), _lib.stream_ptr(dev))

        def argmax():
            fused_ops.greedy_advance(lg, gtok, wi, pos, mask)

        def sampler():
            fused_ops.top_p_sample(lg, gtok.view(-1), rng, 100, 0.8, 1.0, write_index=wi, pos=pos.view(-1), mask=mask)
        res = {k: replay_us(fn, chain) for k, fn in (("lp0", lp0), ("lp20", lp20), ("empty", empty), ("read", read), ("argmax", argmax),
                                                     ("sampler", sampler))}
        for n, st in states.items():
            assert int(st.count.max()) < cap, "a launch found the record full: the time above is not the kernel's"
        out[B] = res["lp20"][0]
        fmt = lambda k: f"{res[k][0]:6.2f} [{res[k][1]:.2f} .. {res[k][2]:.2f}]"
        say(f"   B {B:2d}: n_top 0 {fmt('lp0')}   n_top 20 {fmt('lp20')}   empty launch {fmt('empty')}   "
            f"streaming read of {nbytes / 1e6:.2f} MB {fmt('read')}   arg-max {fmt('argmax')}   sampler {fmt('sampler')}")
        say(f"         n_top 0 / arg-max {res['lp0'][0] / res['argmax'][0]:.2f}   n_top 20 / sampler {res['lp20'][0] / res['sampler'][0]:.2f}   "
            f"n_top 20 / n_top 0 {res['lp20'][0] / res['lp0'][0]:.2f}   read / n_top 0 {res['read'][0] / res['lp0'][0]:.2f}")
    return out


def model_legs(rounds, T, launch_us, say):
    model, cfg = bench_extras._chatglm2_6b(torch, dev, torch.float16)
    for mod in model.modules():
        if hasattr(mod, "prepare"):
            mod.prepare()
    dec = ChatGLMDecoder(None, model)
    prompt = lambda b: [(37 * i + 11 + 101 * b) % cfg.vocab_size for i in range(32)]
    settings = (None, 0, 5)

    def leg(B, greedy, n):
        def run():
            if B == 1:
                out = [list(dec.generate_ids(prompt(0), greedy=greedy, seed=5, max_generated_tokens=T, ignore_eos=True, logprobs=n))]
                recs = [dec.last_logprobs]
            else:
                out = dec.generate_batch_ids([prompt(b) for b in range(B)], greedy=greedy, seed=list(range(B)), max_generated_tokens=T,
                                             ignore_eos=True, logprobs=n)
                recs = dec.last_logprobs
            assert [len(o) for o in out] == [T] * B and dec.last_stats["logprobs"] is (n is not None)
            assert n is None or [len(r) for r in recs] == [T] * B
            return dec.last_stats["gen_tok_per_s"]
        return run

    legs = {}
    for B in (1, 8, 32):
        for mode, greedy in (("greedy", True), ("sampled", False)):
            for n in settings:
                legs[(B, mode, n)] = leg(B, greedy, n)
    for fn in legs.values():                                     # untimed warm-up: layouts, graphs, allocator
        fn()
    res = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            res[k].append(fn())
    med = {k: statistics.median(v) for k, v in res.items()}
    say(f"2. synthetic ChatGLM2-6B int4g32, 32-id prompts, {T} tokens, EOS ignored, generated tok/s after the first token (all rows), "
        f"{rounds} alternated rounds: median [min .. max]")
    say("   on/off = tok/s with logprobs over tok/s without; predicted = step / (step + n_top 20 launch of part 1), step = B / (tok/s off)")
    say("   (the time of the one read of the record at the end is not part of gen tok/s: the last token's time ends before it)")
    for B in (1, 8, 32):
        for mode in ("greedy", "sampled"):
            off = med[(B, mode, None)]
            step_us = B / off * 1e6
            pred = step_us / (step_us + launch_us[B]) if launch_us else float("nan")
            rng = lambda k: f"[{min(res[k]):.1f} .. {max(res[k]):.1f}]"
            line = f"   B {B:2d} {mode:7s}: off {off:8.1f} {rng((B, mode, None))}"
            for n in settings[1:]:
                on = med[(B, mode, n)]
                line += f"   logprobs={n} {on:8.1f} {rng((B, mode, n))} on/off {on / off:.4f} (+{step_us * (off / on - 1):.2f} us)"
            say(line + f"   predicted {pred:.4f} (step {step_us:.1f} us, +{launch_us.get(B, float('nan')):.2f} us)")


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
    say(f"tools/logprobs_bench.py on {torch.cuda.get_device_name(0)}")
    launch_us = launch_alone(a.chain, say)
    if not a.skip_model:
        model_legs(a.rounds, a.tokens, launch_us, say)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

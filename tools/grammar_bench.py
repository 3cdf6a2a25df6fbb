"""Developer tool: what regex-constrained generation (``grammar=``: ``qlinear_grammar_mask``) costs (profiles/grammar_ab.txt).

1. The launch alone under graph replay: fp16 logits, N = 65024, batch 1 / 8 / 32, over a synthetic vocabulary of 65 024 tokens with
   the length distribution of a sentencepiece vocabulary (256 one-byte tokens, then mostly 2 - 9 bytes, a tail up to 20; some empty).
   Every launch of the chain is fed an EMPTY token, so the state stays where it was armed and every launch does the same walk.
   Patterns: a small one (``[A-D]`` at its start: almost every token dies at its first byte), a mid-sized one (a flat JSON object of
   strings and numbers, at its start and INSIDE a string value, where most tokens survive to their last byte - the long walk), a
   counted run of printable characters (the pattern of part 2) and one at GRAMMAR_TABLE_MAX (2048 states x 8 classes: the 32 KB
   table copy per workgroup).  A graph of ``--chain`` launches is replayed; per launch: the median over the replays / chain.  Next to
   it, measured the same way in the same run: the empty launch and the pure streaming read of the bytes a launch touches per row
   (offsets + token bytes; probe kernels of libqlinear_hip_span.so, csrc/probe_kernels.hip), the arg-max launch and the sampler's.
2. Generated tokens per second after the first token on the synthetic 28-layer ChatGLM2-6B int4g32 model
   (``bench_extras._chatglm2_6b``), 32-id prompts, ``--tokens`` tokens: greedy and sampled, batch 1 (``generate_ids``) / 8 / 32
   (``generate_batch_ids``), the grammar off against on, the legs ALTERNATED round by round in one process after an untimed warm-up of
   each.  The pattern is ``[ -~]{3000}``: 3 000 printable bytes before it is complete, so the end token is never allowed within the
   budget and both legs generate ``--tokens`` tokens.

    python tools/grammar_bench.py [--rounds 5] [--tokens 128] [--skip-model] [--out profiles/grammar_ab.txt]

The off path needs no timing: with ``grammar=None`` it issues and replays exactly the launches it did before the feature existed
(tests/test_grammar_gpu.py::test_launch_accounting).
"""
import argparse
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

import bench_extras  # noqa: E402
from chatglm_q_amd import _lib, fused_ops  # noqa: E402
from chatglm_q_amd import grammar as G  # noqa: E402
from chatglm_q_amd.decoder import ChatGLMDecoder  # noqa: E402
from logprobs_bench import REPS, V, dev, probe_lib, replay_us  # noqa: E402

JSON = '\\{("[a-z_]+":("[^"]*"|-?[0-9]+)(,"[a-z_]+":("[^"]*"|-?[0-9]+))*)?\\}'
LIMIT = "x{2031}(a|bb|ccc|dddd|eeeee|ffffff)"
RUN = "[ -~]{3000}"
# token lengths in bytes and their weights: the shape of a sentencepiece vocabulary of Chinese + English text (the byte-fallback pieces
# come on top)
LENGTHS = ((0, 1), (1, 2), (2, 8), (3, 17), (4, 14), (5, 11), (6, 14), (7, 8), (8, 6), (9, 8), (10, 3), (11, 2), (12, 3), (15, 2), (20, 1))


def synthetic_vocab(n=V, seed=1):
    rng = random.Random(seed)
    ascii_chars = bytes(range(0x20, 0x7F))
    cjk = [chr(c).encode() for c in range(0x4E00, 0x4E00 + 3000)]
    toks = [bytes([b]) for b in range(256)]
    lengths, weights = zip(*LENGTHS)
    while len(toks) < n:
        L = rng.choices(lengths, weights)[0]
        if L and L % 3 == 0 and rng.random() < 0.6:                 # whole three-byte characters
            toks.append(b"".join(rng.choice(cjk) for _ in range(L // 3)))
        else:
            first = b" " if L > 1 and rng.random() < 0.5 else b""    # a word with its leading space
            toks.append(first + bytes(rng.choice(ascii_chars[33:59] + ascii_chars[65:91] * 4) for _ in range(L - len(first))))
    rng.shuffle(toks)
    return toks


def launch_alone(chain, vocab, say):
    probes = probe_lib()
    g = torch.Generator().manual_seed(3)
    table = G.token_byte_table(vocab)
    empty_id = vocab.index(b"")
    per_row = 4 * (len(table) + 1) + int(table.bytes.size)
    dfas = {"[A-D]": (G.compile_regex("[A-D]"), b""), "json, start": (G.compile_regex(JSON), b""),
            "json, in a string": (G.compile_regex(JSON), b'{"k":"v'), "printable run": (G.compile_regex(RUN), b"abc"),
            "at the table limit": (G.compile_regex(LIMIT), b"")}
    out = {}
    say(f"1. qlinear_grammar_mask alone, graph of {chain} launches replayed {REPS} times, us per launch: median [min .. max]")
    say(f"   fp16 logits (B, {V}); vocabulary: {len(table)} tokens, {table.bytes.size} bytes ({per_row / 1e6:.2f} MB of offsets + bytes per row);")
    say(f"   GRAMMAR_CHUNK {fused_ops.GRAMMAR_CHUNK}: {-(-V // fused_ops.GRAMMAR_CHUNK)} workgroups per row; every launch is fed an empty token (the state stays)")
    for name, (d, _) in dfas.items():
        say(f"   {name}: {d.n_states} states x {d.n_classes} classes = {d.n_states * d.n_classes * 2} bytes of table per workgroup")
    for B in (1, 8, 32):
        lg = (torch.randn(B, V, generator=g) * 3).half().to(dev)
        tok = torch.full((B,), empty_id, dtype=torch.int64, device=dev)
        states, survive = {}, {}
        for name, (d, prefix) in dfas.items():
            st = fused_ops.GrammarState(B, table, dev).arm([d] * B, [empty_id] * B)
            s = d.step(0, prefix)
            assert s >= 0
            st.state.fill_(s)
            states[name] = (st, s)
            survive[name] = sum(1 for t in vocab if t and d.step(s, t) >= 0)
        nbytes = (B * per_row + 15) // 16 * 16
        region = torch.zeros(nbytes // 4, dtype=torch.int32, device=dev)
        sink = torch.zeros(int(probes.qlinear_probe_read_waves(nbytes)) + 64, dtype=torch.int32, device=dev)
        gtok = torch.zeros(B, 1, dtype=torch.int64, device=dev)
        wi = torch.zeros(1, dtype=torch.int64, device=dev)
        pos = torch.zeros(B, 1, dtype=torch.int64, device=dev)
        mask = torch.zeros(B, 1, 4096, dtype=torch.float32, device=dev)
        rng = fused_ops.new_rng_state(B, 5, dev)
        bodies = {name: (lambda st=st: fused_ops.grammar_mask(lg, st, tok)) for name, (st, _) in states.items()}
        bodies["empty"] = lambda: probes.qlinear_probe_empty(256, _lib.stream_ptr(dev))
        bodies["read"] = lambda: probes.qlinear_probe_read(region.data_ptr(), nbytes, sink.data_ptr(), _lib.stream_ptr(dev))
        bodies["argmax"] = lambda: fused_ops.greedy_advance(lg, gtok, wi, pos, mask)
        bodies["sampler"] = lambda: fused_ops.top_p_sample(lg, gtok.view(-1), rng, 100, 0.8, 1.0, write_index=wi, pos=pos.view(-1), mask=mask)
        res = {}
        for k, fn in bodies.items():
            lg.normal_(0, 3)                                     # (the selection yardsticks read finite logits)
            res[k] = replay_us(fn, chain)
        for name, (st, s) in states.items():
            assert st.states() == [s] * B and st.ticket.tolist() == [0] * B, "a launch moved the state: the time above is not one walk's"
        out[B] = res["printable run"][0]
        fmt = lambda k: f"{res[k][0]:6.2f} [{res[k][1]:.2f} .. {res[k][2]:.2f}]"
        say(f"   B {B:2d}: " + "   ".join(f"{name} ({survive[name]} ids survive) {fmt(name)}" for name in dfas))
        say(f"         empty launch {fmt('empty')}   streaming read of {nbytes / 1e6:.2f} MB {fmt('read')}   arg-max {fmt('argmax')}   sampler {fmt('sampler')}")
        worst = max(res[name][0] for name in dfas)
        say(f"         slowest pattern / sampler {worst / res['sampler'][0]:.2f}   / arg-max {worst / res['argmax'][0]:.2f}   / read {worst / res['read'][0]:.2f}   "
            f"/ empty {worst / res['empty'][0]:.2f}   [A-D] / empty {res['[A-D]'][0] / res['empty'][0]:.2f}")
    return out


def model_legs(rounds, T, launch_us, vocab, say):
    model, cfg = bench_extras._chatglm2_6b(torch, dev, torch.float16)
    for mod in model.modules():
        if hasattr(mod, "prepare"):
            mod.prepare()
    table = G.token_byte_table(vocab).padded(cfg.vocab_size)
    eos = vocab.index(b"")
    off_dec, on_dec = ChatGLMDecoder(None, model), ChatGLMDecoder(None, model, eos_token_id=eos, token_bytes=table)
    dfa = G.compile_regex(RUN)
    prompt = lambda b: [(37 * i + 11 + 101 * b) % cfg.vocab_size for i in range(32)]

    def leg(B, greedy, on):
        dec = on_dec if on else off_dec
        kw = dict(grammar=dfa) if on else dict(ignore_eos=True)

        def run():
            if B == 1:
                out = [list(dec.generate_ids(prompt(0), greedy=greedy, seed=5, max_generated_tokens=T, **kw))]
            else:
                out = dec.generate_batch_ids([prompt(b) for b in range(B)], greedy=greedy, seed=list(range(B)), max_generated_tokens=T, **kw)
            assert [len(o) for o in out] == [T] * B and dec.last_stats["grammar"] is on
            if on:
                assert all(dfa.step(0, table.join(o)) >= 0 for o in out), "a constrained row left the pattern"
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
    say(f"2. synthetic ChatGLM2-6B int4g32, 32-id prompts, {T} tokens, generated tok/s after the first token (all rows), "
        f"{rounds} alternated rounds: median [min .. max]")
    say(f"   on = grammar {RUN!r} ({dfa.n_states} states x {dfa.n_classes} classes); on/off = tok/s with the grammar over tok/s without; "
        "predicted = step / (step + 'printable run' launch of part 1), step = B / (tok/s off)")
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
    say(f"tools/grammar_bench.py on {torch.cuda.get_device_name(0)}")
    vocab = synthetic_vocab()
    launch_us = launch_alone(a.chain, vocab, say)
    if not a.skip_model:
        model_legs(a.rounds, a.tokens, launch_us, vocab, say)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""Developer tool: what JSON-constrained generation (a ``grammar.BytePDA``: ``qlinear_pda_mask``) costs (profiles/grammar_pda_ab.txt).

1. The launch alone under graph replay, measured as tools/grammar_bench.py measures the DFA launch and over the same synthetic
   vocabulary of 65 024 tokens: fp16 logits, N = 65024, batch 1 / 8 / 32, every launch fed an EMPTY token (the configuration stays).
   ``json_grammar()`` at its start and inside a string value at depth 3; a lifted DFA (``[A-D]`` and grammar_bench's flat-JSON pattern,
   at its start and inside a string value) through ``qlinear_pda_mask`` against the SAME DFA through ``qlinear_grammar_mask`` - that
   ratio is the price of the stack machinery on equal work; the empty launch, the arg-max and the sampler launches beside them.  All
   legs in one run, ALTERNATED: ``--passes`` passes over all legs, each leg's figure the median over the passes of its replay median.
2. Generated tokens per second after the first token on the synthetic 28-layer ChatGLM2-6B int4g32 model, 32-id prompts, ``--tokens``
   tokens, batch 1 (``generate_ids``) and 8 (``generate_batch_ids``), greedy: ``grammar=json_grammar(whitespace=True, max_depth=64)`` on
   against off, the legs alternated round by round after an untimed warm-up of each.  The on leg's automaton has its accept flags
   cleared - the same table, the same walks, but the end token is never allowed, and behind a complete document whitespace still is -
   so both legs generate ``--tokens`` tokens.

    python tools/pda_bench.py [--rounds 3] [--tokens 128] [--passes 3] [--skip-model] [--out profiles/grammar_pda_ab.txt]
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
from chatglm_q_amd import grammar as G  # noqa: E402
from chatglm_q_amd.decoder import ChatGLMDecoder  # noqa: E402
from grammar_bench import JSON, synthetic_vocab  # noqa: E402
from logprobs_bench import REPS, V, dev, probe_lib, replay_us  # noqa: E402


def launch_alone(chain, passes, vocab, say):
    probes = probe_lib()
    g = torch.Generator().manual_seed(3)
    table = G.token_byte_table(vocab)
    empty_id = vocab.index(b"")
    js = G.json_grammar()
    dfas = {"[A-D]": (G.compile_regex("[A-D]"), b""), "flat json, start": (G.compile_regex(JSON), b""),
            "flat json, in a string": (G.compile_regex(JSON), b'{"k":"v')}
    pdas = {"json_grammar, start": (js, b""), "json_grammar, in a string at depth 3": (js, b'{"k":[{"k":"v')}
    say(f"1. the launch alone, graph of {chain} launches replayed {REPS} times, {passes} alternated passes over all legs, us per launch: "
        "median of the passes' medians [min .. max of the passes]")
    say(f"   fp16 logits (B, {V}); vocabulary: {len(table)} tokens, {table.bytes.size} bytes; every launch is fed an empty token")
    say(f"   json_grammar(): {js.n_states} states x {js.n_syms + 1} tops x {js.n_classes} classes = {js.table.size * 2} bytes of table per workgroup")
    for B in (1, 8, 32):
        lg = (torch.randn(B, V, generator=g) * 3).half().to(dev)
        tok = torch.full((B,), empty_id, dtype=torch.int64, device=dev)
        bodies, held, survive = {}, [], {}
        for name, (d, prefix) in dfas.items():
            s = d.step(0, prefix)
            assert s >= 0
            gst = fused_ops.GrammarState(B, table, dev).arm([d] * B, [empty_id] * B)
            gst.state.fill_(s)
            pst = fused_ops.PdaState(B, table, dev).arm([d] * B, [empty_id] * B)
            pst.state.fill_(s)
            held.append((gst, pst, s))
            bodies["dfa " + name] = lambda st=gst: fused_ops.grammar_mask(lg, st, tok)
            bodies["lifted " + name] = lambda st=pst: fused_ops.pda_mask(lg, st, tok)
            survive[name] = sum(1 for t in vocab if t and d.step(s, t) >= 0)
        for name, (p, prefix) in pdas.items():
            c = p.step(p.start, prefix)
            assert c is not None
            pst = fused_ops.PdaState(B, table, dev).arm([p] * B, [empty_id] * B)
            pst.state.fill_(c[0])
            pst.depth.fill_(len(c[1]))
            pst.stack[:, :len(c[1])] = torch.tensor(c[1], dtype=torch.uint8, device=dev)
            held.append((None, pst, c[0]))
            bodies[name] = lambda st=pst: fused_ops.pda_mask(lg, st, tok)
            survive[name] = sum(1 for t in vocab if t and p.step(c, t, window=G.PDA_LOCAL_MAX) is not None)
        gtok = torch.zeros(B, 1, dtype=torch.int64, device=dev)
        wi = torch.zeros(1, dtype=torch.int64, device=dev)
        pos = torch.zeros(B, 1, dtype=torch.int64, device=dev)
        mask = torch.zeros(B, 1, 4096, dtype=torch.float32, device=dev)
        rng = fused_ops.new_rng_state(B, 5, dev)
        bodies["empty"] = lambda: probes.qlinear_probe_empty(256, _lib.stream_ptr(dev))
        bodies["argmax"] = lambda: fused_ops.greedy_advance(lg, gtok, wi, pos, mask)
        bodies["sampler"] = lambda: fused_ops.top_p_sample(lg, gtok.view(-1), rng, 100, 0.8, 1.0, write_index=wi, pos=pos.view(-1), mask=mask)
        runs = {k: [] for k in bodies}
        for _ in range(passes):
            for k, fn in bodies.items():
                lg.normal_(0, 3)                                 # (the selection yardsticks read finite logits)
                runs[k].append(replay_us(fn, chain)[0])
        for gst, pst, s in held:
            assert pst.states() == [s] * B and pst.ticket.tolist() == [0] * B, "a launch moved the state: the time above is not one walk's"
            assert gst is None or (gst.states() == [s] * B and gst.ticket.tolist() == [0] * B)
        fmt = lambda k: f"{statistics.median(runs[k]):6.2f} [{min(runs[k]):.2f} .. {max(runs[k]):.2f}]"
        med = lambda k: statistics.median(runs[k])
        say(f"   B {B:2d}: " + "   ".join(f"{name} ({survive[name]} ids survive) {fmt(name)}" for name in pdas))
        for name in dfas:
            say(f"         {name} ({survive[name]} ids survive): qlinear_grammar_mask {fmt('dfa ' + name)}   lifted, qlinear_pda_mask {fmt('lifted ' + name)}   "
                f"lifted / dfa {med('lifted ' + name) / med('dfa ' + name):.3f}")
        say(f"         empty launch {fmt('empty')}   arg-max {fmt('argmax')}   sampler {fmt('sampler')}")


def model_legs(rounds, T, vocab, say):
    model, cfg = bench_extras._chatglm2_6b(torch, dev, torch.float16)
    for mod in model.modules():
        if hasattr(mod, "prepare"):
            mod.prepare()
    table = G.token_byte_table(vocab).padded(cfg.vocab_size)
    eos = vocab.index(b"")
    off_dec, on_dec = ChatGLMDecoder(None, model), ChatGLMDecoder(None, model, eos_token_id=eos, token_bytes=table)
    full = G.json_grammar(whitespace=True, max_depth=G.PDA_DEPTH_MAX)
    js = G.BytePDA(full.class_of, full.table, 0 * full.accept, full.n_syms, full.max_depth, name="json, never accepting")
    prompt = lambda b: [(37 * i + 11 + 101 * b) % cfg.vocab_size for i in range(32)]

    def leg(B, on):
        dec = on_dec if on else off_dec
        kw = dict(grammar=js) if on else dict(ignore_eos=True)

        def run():
            if B == 1:
                out = [list(dec.generate_ids(prompt(0), greedy=True, max_generated_tokens=T, **kw))]
            else:
                out = dec.generate_batch_ids([prompt(b) for b in range(B)], greedy=True, max_generated_tokens=T, **kw)
            assert dec.last_stats["grammar"] is on
            if on:
                for o in out:
                    c = js.start
                    for i in o:
                        c = js.step(c, table.token(i), window=G.PDA_LOCAL_MAX)
                    assert c is not None, "a constrained row left the language"
            assert [len(o) for o in out] == [T] * B
            return dec.last_stats["gen_tok_per_s"]
        return run

    legs = {(B, on): leg(B, on) for B in (1, 8) for on in (False, True)}
    for fn in legs.values():                                     # untimed warm-up: layouts, graphs, allocator
        fn()
    res = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            res[k].append(fn())
    say(f"2. synthetic ChatGLM2-6B int4g32, 32-id prompts, {T} tokens, greedy, generated tok/s after the first token (all rows), "
        f"{rounds} alternated rounds: median [min .. max]; on = grammar=json_grammar(whitespace=True, max_depth={G.PDA_DEPTH_MAX}) with its accept flags cleared")
    for B in (1, 8):
        off, on = statistics.median(res[(B, False)]), statistics.median(res[(B, True)])
        rng = lambda k: f"[{min(res[k]):.1f} .. {max(res[k]):.1f}]"
        say(f"   B {B}: off {off:8.1f} {rng((B, False))}   on {on:8.1f} {rng((B, True))}   on/off {on / off:.4f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--tokens", type=int, default=128)
    ap.add_argument("--chain", type=int, default=64)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"tools/pda_bench.py on {torch.cuda.get_device_name(0)}")
    vocab = synthetic_vocab()
    launch_alone(a.chain, a.passes, vocab, say)
    if not a.skip_model:
        model_legs(a.rounds, a.tokens, vocab, say)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""Developer tool: what scoring on the session path is worth against the composed route (profiles/score_logprob_ab.txt).

Leg 1 - the kernel: ``fused_ops.token_logprob`` on blocks of 512 / 2048 / 8192 rows x 65024 fp16 logits against the composed torch
tail on the SAME tensor (``.float()`` + ``F.cross_entropy(reduction="none")``: what ``ChatGLM2Model.forward(labels=)`` runs) and
against the pure streaming read of the same bytes (``qlinear_probe_read`` of the span build of the library: the floor of a
launch that reads a block once).  Leg 2 - the call: ``DecodeSession.score`` on the synthetic 28-layer ChatGLM2-6B int4g32 model
(``fill_synthetic_``) at 20 x 256 and 4 x 2048 ids against ``model(input_ids, attention_mask, labels)``, tokens/s and
``torch.cuda.max_memory_allocated`` above the resident model.

Device events around every timed group, warmed up, the routes ALTERNATED round by round in one process; per route the median of
the rounds and their [min .. max].  Run the command twice for the run-to-run spread.

    python tools/score_bench.py [--rounds 5] [--skip-model]
"""
import argparse
import ctypes
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import bench_extras  # noqa: E402
from chatglm_q_amd import _lib, fused_ops  # noqa: E402
from chatglm_q_amd.decoder import DecodeSession  # noqa: E402

dev = torch.device("cuda:0")
V = 65024


def timed(fn, reps):
    """Mean device time of `reps` back-to-back calls, microseconds (one event pair around the group)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def summary(xs):
    return f"{statistics.median(xs):10.1f} [{min(xs):.1f} .. {max(xs):.1f}]"


def probe_lib():
    path = os.path.join(os.path.dirname(_lib.LIB_PATH), "libqlinear_hip_span.so")
    if not os.path.exists(path):
        return None
    lib = ctypes.CDLL(path)
    lib.qlinear_probe_read.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
    lib.qlinear_probe_read_waves.restype = ctypes.c_int64
    lib.qlinear_probe_read_waves.argtypes = [ctypes.c_int64]
    return lib


def kernel_leg(rounds):
    print(f"== leg 1: blocks of R x {V} fp16 logits; microseconds per call: median [min .. max] over {rounds} alternated rounds")
    probe = probe_lib()
    for R in (512, 2048, 8192):
        g = torch.Generator(device=dev).manual_seed(R)
        x = (torch.randn(R, V, device=dev, generator=g) * 3).half()
        t = torch.randint(0, V, (R,), device=dev, generator=g)
        nbytes = x.numel() * 2
        sink = torch.zeros(int(probe.qlinear_probe_read_waves(nbytes)) + 64, dtype=torch.int32, device=dev) if probe else None
        st = _lib.stream_ptr(dev)
        routes = {
            "kernel": (lambda: fused_ops.token_logprob(x, t), 20),
            "composed": (lambda: F.cross_entropy(x.float(), t, reduction="none"), 4),
        }
        if probe:
            routes["pure_read"] = (lambda: probe.qlinear_probe_read(x.data_ptr(), nbytes, sink.data_ptr(), st), 20)
        got = fused_ops.token_logprob(x, t)
        want = -F.cross_entropy(x.float(), t, reduction="none")
        assert torch.allclose(got, want, rtol=0, atol=1e-4), (got - want).abs().max()
        for fn, reps in routes.values():                         # warm-up
            timed(fn, 2)
        times = {k: [] for k in routes}
        for _ in range(rounds):
            for k, (fn, reps) in routes.items():
                times[k].append(timed(fn, reps))
        med = {k: statistics.median(v) for k, v in times.items()}
        for k in routes:
            print(f"R={R:5d} {k:10s} {summary(times[k])} us   {nbytes / med[k] / 1e6:7.3f} TB/s of logits bytes")
        line = f"R={R:5d} kernel vs composed: {med['composed'] / med['kernel']:.2f}x faster"
        if probe:
            line += f"; kernel at {med['pure_read'] / med['kernel']:.2f} of the pure read of the same bytes"
        print(line, flush=True)
        del x


def model_leg(rounds):
    model, cfg = bench_extras._chatglm2_6b(torch, dev, torch.float16)
    print(f"== leg 2: synthetic 28-layer ChatGLM2-6B int4g32, fp16; ms per call: median [min .. max] over {rounds} alternated rounds; "
          f"peak = max_memory_allocated above what is resident before the call")
    for B, S in ((20, 256), (4, 2048)):
        g = torch.Generator().manual_seed(B)
        ids = torch.randint(0, cfg.vocab_size, (B, S), generator=g)
        attn = torch.ones(B, S, dtype=torch.long)
        for b in range(1, B):                                    # left padded, unequal lengths (row 0 is full width)
            attn[b, : (b * S) // (3 * B)] = 0
        labels = ids.masked_fill(~attn.bool(), -100)
        ids_d, attn_d, labels_d = ids.to(dev), attn.to(dev), labels.to(dev)
        sess = DecodeSession(model, B, S, use_graph=False)
        out = {}

        def run_score():
            out["score"] = sess.reset().score(ids_d, attention_mask=attn_d, labels=labels_d).loss

        def run_forward():
            with torch.no_grad():
                out["forward"] = model(input_ids=ids_d, attention_mask=attn_d, labels=labels_d)[0]

        routes = {"score()": run_score, "forward(labels=)": run_forward}
        for fn in routes.values():                               # warm-up: derived layouts, allocator pools
            fn()
        torch.cuda.synchronize()
        print(f"B x S = {B} x {S}: loss score() {float(out['score']):.5f}, forward(labels=) {float(out['forward']):.5f}")
        times, peaks = {k: [] for k in routes}, {k: 0 for k in routes}
        for _ in range(rounds):
            for k, fn in routes.items():
                out.clear()
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                times[k].append(timed(fn, 1) / 1e3)
                peaks[k] = max(peaks[k], torch.cuda.max_memory_allocated() - base)
        tokens = int(attn.sum())
        med = {k: statistics.median(v) for k, v in times.items()}
        for k in routes:
            print(f"B x S = {B} x {S} {k:17s} {summary(times[k])} ms   {tokens / med[k] * 1e3:9.0f} tok/s   peak {peaks[k] / 2**20:8.1f} MiB")
        print(f"B x S = {B} x {S} score() vs forward(labels=): {med['forward(labels=)'] / med['score()']:.2f}x the tokens/s, "
              f"{peaks['score()'] / peaks['forward(labels=)']:.3f} of the peak bytes", flush=True)
        del sess


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-model", action="store_true")
    args = ap.parse_args()
    print(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}")
    kernel_leg(args.rounds)
    if not args.skip_model:
        model_leg(args.rounds)

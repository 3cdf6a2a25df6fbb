"""Developer tool: what GPTQ costs per layer with the block kernel (csrc/gptq.hip, ``use_kernel=True``) against the composed torch
path (``use_kernel=False``: the reference's column-by-column loop, about a dozen small launches per input column) on the same GPU
(profiles/gptq_ab.txt).

Shapes (out x in): ChatGLM2-6B's o_proj 4096 x 4096, qkv_proj 4608 x 4096, w_in 27392 x 4096, w_out 4096 x 13696 and lm_head
65024 x 4096, int4g32 and int8, blocksize 128.  Weights are seeded normal values, the Hessian comes from ``--samples`` seeded
correlated input rows pushed through the quantizer's own hook.

Per shape and path:
  total        ``quantize_weight()`` end to end, host clock around a device synchronise, median of ``--reps`` (one untimed run first)
  factor       dead columns + damping + the two Cholesky factorisations + the inverse (the same torch calls on both paths)
  blocks       the walks inside the blocks: device events around every ``fused_ops.gptq_block`` call of one pass, summed
  gemms        the updates of the columns right of each block (``W[:, i2:] -= Err @ Hinv[i1:i2, i2:]``), likewise
  us / block   blocks / number of blocks: on the kernel path one launch of ``qlinear_gptq_block``
and the two paths' results compared by rows (rows with any differing integer code).

    python tools/gptq_bench.py [--reps 3] [--samples 4096] [--shapes 4096x4096,...] [--skip-composed] [--out profiles/gptq_ab.txt]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from torch import nn  # noqa: E402

from chatglm_q_amd import _lib, fused_ops  # noqa: E402
from chatglm_q_amd.int4 import quantizer as q4  # noqa: E402
from chatglm_q_amd.int8 import quantizer as q8  # noqa: E402

dev = torch.device("cuda:0")
SHAPES = "4096x4096,4608x4096,27392x4096,4096x13696,65024x4096"
BLOCK = 128


def make_quantizer(mod, rows, cols, samples, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    layer = nn.Linear(cols, rows, bias=False, device=dev)
    with torch.no_grad():
        layer.weight.copy_(torch.randn((rows, cols), generator=g, device=dev) * 0.02)
    q = mod.GPTQLinearQuantizer(layer)
    mix = torch.randn((64, cols), generator=g, device=dev)
    with torch.no_grad():
        for _ in range(max(1, samples // 1024)):
            x = torch.randn((1024, 64), generator=g, device=dev) @ mix * 0.25 + torch.randn((1024, cols), generator=g, device=dev) * 0.5
            layer(x)
    q.remove_hook()
    return q


def timed_stages(q, hessian0, bits, use_kernel):
    """One pass of quantize_weight's stages with a clock on each: (factor ms, blocks ms, gemms ms, n_blocks, launches)."""
    q.hessian.copy_(hessian0)
    weight = q.layer.weight.detach().clone()
    if bits == 8:
        scale = q8.quantize_int8(weight)[1].contiguous()
    else:
        scale = torch.empty((q.n_columns // 32, q.n_rows), device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    hinv = q._factor(weight, .01).contiguous()
    torch.cuda.synchronize()
    factor_ms = (time.perf_counter() - t0) * 1e3
    marks = []
    before = _lib.launch_count()
    for i1 in range(0, q.n_columns, BLOCK):
        i2 = min(i1 + BLOCK, q.n_columns)
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        _, Err, _ = fused_ops.gptq_block(weight, i1, i2 - i1, hinv, bits, scale, 32, use_kernel=use_kernel)
        e[1].record()
        if i2 < q.n_columns:
            weight[:, i2:] -= Err.matmul(hinv[i1:i2, i2:])
        e[2].record()
        marks.append(e)
    torch.cuda.synchronize()
    launches = _lib.launch_count() - before
    blocks_ms = sum(e[0].elapsed_time(e[1]) for e in marks)
    gemms_ms = sum(e[1].elapsed_time(e[2]) for e in marks)
    return factor_ms, blocks_ms, gemms_ms, len(marks), launches


def total_ms(q, hessian0, bits, use_kernel, reps):
    times, out = [], None
    for i in range(reps + 1):
        q.hessian.copy_(hessian0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = q.quantize_weight(use_kernel=use_kernel)          # ends in .item(): synchronised
        torch.cuda.synchronize()
        if i:
            times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), min(times), max(times), out


def rows_differing(bits, a, b):
    (ga, sa), (gb, sb) = a, b
    if bits == 8:
        ca, cb = torch.round(ga / sa[:, None]), torch.round(gb / sb[:, None])
    else:
        ca = torch.round(ga / sa.t().repeat_interleave(32, dim=1))
        cb = torch.round(gb / sb.t().repeat_interleave(32, dim=1))
    return int((ca != cb).any(dim=1).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--skip-composed", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/gptq_bench.py measures on the GPU; there is none")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"GPTQ quantize_weight per layer, blocksize {BLOCK}, {args.samples} calibration rows, {torch.cuda.get_device_name(0)}")
    say("ms: total = median [min .. max] of %d; factor / blocks / gemms = one pass with a clock per stage" % args.reps)
    say(f"{'shape':>13} {'fmt':>5} {'path':>9} {'total ms':>28} {'factor':>9} {'blocks':>10} {'gemms':>9} {'n':>4} {'us/block':>10} {'launches':>8}")
    for shape in args.shapes.split(","):
        rows, cols = (int(v) for v in shape.lower().split("x"))
        for fmt, mod, bits in (("int4", q4, 4), ("int8", q8, 8)):
            q = make_quantizer(mod, rows, cols, args.samples, 1000 + bits)
            hessian0 = q.hessian.clone()
            results = {}
            for path, use_kernel in (("kernel", True), ("composed", False)):
                if not use_kernel and args.skip_composed:
                    continue
                med, lo, hi, out = total_ms(q, hessian0, bits, use_kernel, args.reps)
                f_ms, b_ms, g_ms, n, launches = timed_stages(q, hessian0, bits, use_kernel)
                results[path] = (med, b_ms, (out[0], out[1]))
                say(f"{shape:>13} {fmt:>5} {path:>9} {med:10.1f} [{lo:7.1f} .. {hi:7.1f}] {f_ms:9.1f} {b_ms:10.2f} {g_ms:9.2f} {n:4d} "
                    f"{b_ms * 1e3 / n:10.1f} {launches:8d}")
            if len(results) == 2:
                k, c = results["kernel"], results["composed"]
                say(f"{'':>13} {fmt:>5} composed / kernel: total {c[0] / k[0]:.2f}x, blocks {c[1] / k[1]:.1f}x; rows with a differing code: "
                    f"{rows_differing(bits, k[2], c[2])} of {rows}")
            del q, hessian0, results
            torch.cuda.empty_cache()
    if args.out:
        path = os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

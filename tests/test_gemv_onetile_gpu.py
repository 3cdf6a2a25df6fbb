"""The one-tile one-row int4g32 GEMV (w4_packed.hip, ONE_TILE: straight-line body, activation work in front of the weight waits, 2 or 4
columns per wave) against the tile-loop kernel it replaces for K slices of one 64-group tile.

Every case runs the call twice in one process - default dispatch, then QLINEAR_DISPATCH=noonetile - and wants the two results BIT FOR BIT
equal (the per-column arithmetic, the reductions, the K-slice add order and the rounding are the same code), checks which kernel ran through
the library's launch counter of the one-tile kernel, and compares with the oracle at the tolerance tests/test_parity_gpu.py uses for the
dtype and the arithmetic mode (1e-3; 4e-3 for bf16 in the default exact-dequant mode).  For the fused entries the oracle multiplies the row
that the library's separate prologue ops (fused_ops.rmsnorm / add_rmsnorm / silu_mul) produce.

The oracle figure is a relative L2 error, and that tolerance was set on matrices of thousands of outputs: over the 2 - 8 outputs of the
narrow shapes it is decided by whether ONE output crosses a rounding boundary of the dtype (one bf16 ulp of one output in eight is
1.4e-3 .. 2.8e-3 by itself: over one row of 8 columns the tile-loop kernel itself measures up to 4.95e-3 in bf16's default arithmetic).
So a narrow shape runs ROWS_NARROW different activation rows - one one-row launch each, every one compared bit for bit - and
the relative L2 error is taken over all their outputs together, at the unchanged tolerance.

Shapes: the smallest that reach each branch -
  K=4096 N=8     2 K slices, one tile per wave, a block with waves that shadow quad 0
  K=4096 N=6     partial quad: element-wise epilogue; with 2 columns per wave a wave with one live column
  K=4096 N=2     partial quad; with 2 columns per wave a wave with no live column
  K=4096 N=4608  qkv_proj: 2.25 blocks per CU (4.5 with 2 columns per wave)
  K=2048 N=8     64 groups: one slice, no K combine
  K=1056 N=8     33 groups: masked lanes
  K=8192 N=8     256 groups: 4 slices (4 columns per wave: a quad's 8 two-column waves would not fit a block)
  K=4160 N=8     130 groups: two tiles per wave - must stay on the tile-loop kernel
"""
import functools

import pytest
import torch

from oracle import qlinear_oracle as O

pytestmark = pytest.mark.gpu

from chatglm_q_amd import _lib  # noqa: E402
from chatglm_q_amd import fused_ops as F_  # noqa: E402
from chatglm_q_amd.int4 import hip_ops as h4  # noqa: E402

DEV = "cuda:0"
TDT = {"f16": torch.float16, "bf16": torch.bfloat16}
REL, REL_DEFAULT_BF16 = 1e-3, 4e-3          # tests/test_parity_gpu.py: REL[dt], and the documented bf16 exact-dequant exception
SHAPES = [(4096, 8), (4096, 6), (4096, 2), (4096, 4608), (2048, 8), (1056, 8), (8192, 8), (4160, 8)]
ONE_TILE = {s: s != (4160, 8) for s in SHAPES}
ENTRIES = ["plain", "bias", "residual", "residual_bias", "addnorm_delta", "addnorm", "norm", "silu"]   # norm: no delta and no hout (PRO_NORM)
EPS = 1e-5
ROWS_NARROW = 32


def t2n(t):
    t = t.detach().cpu()
    return t.float().numpy() if t.dtype == torch.bfloat16 else t.numpy()


@functools.lru_cache(maxsize=None)
def weights(K, N, dt):
    g = torch.Generator().manual_seed(K * 5 + N)
    qw = torch.randint(0, 256, (K // 2, N), dtype=torch.uint8, generator=g)
    sc = (torch.rand((K // 32, N), generator=g) * 0.02 + 0.002).to(TDT[dt])
    bias = (torch.randn(N, generator=g) * 0.1).to(TDT[dt])
    qd, sd = qw.to(DEV), sc.to(DEV)
    return qw, sc, bias, qd, sd, h4.repack_w4g32(qd, sd), bias.to(DEV)


@pytest.fixture(autouse=True)
def dispatch_as_the_environment_says():
    """Set up first, so finalised after monkeypatch has put QLINEAR_DISPATCH back: the library's parsed flags follow the variable again."""
    yield
    _lib.get_lib().qlinear_dispatch_reload()


def onetile_launches():
    return int(_lib.get_lib().qlinear_w4g32_onetile_launches())


def both_kernels(call, monkeypatch, one_tile):
    """call() under the default dispatch and under noonetile; the launch counter says which kernel served each."""
    lib = _lib.get_lib()
    lib.qlinear_dispatch_reload()
    n0 = onetile_launches()
    new = call()
    n1 = onetile_launches()
    try:
        monkeypatch.setenv("QLINEAR_DISPATCH", "noonetile")
        lib.qlinear_dispatch_reload()
        assert lib.qlinear_dispatch_flags() & 256
        old = call()
        n2 = onetile_launches()
    finally:
        monkeypatch.delenv("QLINEAR_DISPATCH")
        lib.qlinear_dispatch_reload()
    torch.cuda.synchronize()
    assert n1 - n0 == one_tile, "the default dispatch took the wrong kernel"
    assert n2 - n1 == 0, "noonetile still launched the one-tile kernel"
    return new, old


def run_entry(entry, K, N, dt, strict, row=0):
    """-> (call, oracle reference as a torch tensor of the dtype); call() returns a tuple of tensors to compare bit for bit."""
    tdt = TDT[dt]
    qw, sc, bias_c, qd, sd, packed, bias_d = weights(K, N, dt)
    g = torch.Generator().manual_seed(K + N + len(entry) + 1000 * row)
    width = 2 * K if entry == "silu" else K
    a = torch.randn((1, 1, width), generator=g).to(tdt).to(DEV)
    use_bias = entry in ("bias", "residual_bias", "addnorm_delta")
    bd, bc = (bias_d, bias_c) if use_bias else (None, None)

    def oracle(x):
        return torch.from_numpy(O.w4_matmul(t2n(x.reshape(1, K)), qw.numpy(), t2n(sc), None if bc is None else t2n(bc), dtype=dt)).to(tdt)

    if entry in ("plain", "bias"):
        return (lambda: (h4.w4_forward(a.reshape(1, K), qd, sd, bd, packed, strict=strict),)), oracle(a)
    if entry.startswith("residual"):
        res = torch.randn((1, 1, N), generator=g).to(tdt)
        res_d = res.to(DEV)
        return (lambda: (h4.w4_forward_residual(a, packed, N, bd, res_d, strict=strict),)), oracle(a) + res.reshape(1, N)
    if entry == "silu":
        return (lambda: (h4.w4_forward_fused(_lib.PRO_SILU, a, packed, N, bd, strict=strict),)), oracle(F_.silu_mul(a, K))
    w = (1 + 0.1 * torch.randn(K, generator=g)).to(tdt).to(DEV)
    delta = torch.randn((1, 1, K), generator=g).to(tdt).to(DEV) if entry == "addnorm_delta" else None

    def call():
        if entry == "norm":
            return (h4.w4_forward_fused(_lib.PRO_ADDNORM, a, packed, N, bd, None, w, None, EPS, strict=strict),)
        hout = torch.empty_like(a)
        return h4.w4_forward_fused(_lib.PRO_ADDNORM, a, packed, N, bd, delta, w, hout, EPS, strict=strict), hout

    x = F_.rmsnorm(a, w, EPS) if delta is None else F_.add_rmsnorm(a, delta, w, EPS)[1]
    return call, oracle(x)


@pytest.mark.parametrize("strict", [False, True], ids=["default", "strict"])
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("K,N", SHAPES)
def test_onetile_equals_tile_loop_and_oracle(K, N, entry, dt, strict, monkeypatch):
    rows = ROWS_NARROW if N <= 8 else 1
    calls, refs = zip(*[run_entry(entry, K, N, dt, strict, r) for r in range(rows)])
    new, old = both_kernels(lambda: [c() for c in calls], monkeypatch, rows if ONE_TILE[(K, N)] else 0)
    for xs, ys in zip(new, old):
        for x, y in zip(xs, ys):
            assert torch.equal(x, y), (K, N, entry, dt, strict, (x != y).sum().item())
    tol = REL_DEFAULT_BF16 if (dt == "bf16" and not strict) else REL
    err = O.rel_l2(t2n(torch.cat([xs[0].reshape(1, N) for xs in new])), t2n(torch.cat([r.reshape(1, N) for r in refs])))
    print(f"rel_l2 {K}x{N} {entry} {dt} {'strict' if strict else 'default'}: {err:.3e} (bound {tol:.0e})")
    assert err <= tol, (K, N, entry, dt, strict, err)


def test_onetile_graph_replay_equals_eager():
    """The one-tile launch captured in a graph and replayed (how the decode step and the benchmark run it) computes what it computes eagerly."""
    K, N = 4096, 4608
    _, _, _, qd, sd, packed, bias_d = weights(K, N, "f16")
    a = torch.randn((1, K), generator=torch.Generator().manual_seed(5)).half().to(DEV)
    n0 = onetile_launches()
    eager = h4.w4_forward(a, qd, sd, bias_d, packed, strict=False)
    assert onetile_launches() - n0 == 1
    stream = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(stream):
        h4.w4_forward(a, qd, sd, bias_d, packed, strict=False)       # warm-up outside the capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            out = h4.w4_forward(a, qd, sd, bias_d, packed, strict=False)
        out.zero_()
        graph.replay()
        stream.synchronize()
    assert torch.equal(out, eager)

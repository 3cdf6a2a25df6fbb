"""K-complete geometry of the one-tile one-row int4g32 GEMV (w4_packed.hip, body parameter KC) against the tile-loop kernel, BIT FOR BIT.
At two K slices a wave owns CC whole columns - both slices - instead of two columns of one slice: no sums in LDS, no second barrier, no
owner wave; lane 0 of every wave with a live column rounds and stores its own (CC = 1: a 2-byte store; CC = 2: a 4-byte store when both
columns are live and the output is 4-byte aligned, element-wise otherwise).

PRODUCT_KC is what libqlinear_hip.so's default dispatch runs at two K slices, the outcome of profiles/gemv_kcomplete_ab.txt: 0 = the quad
combine of the two-column waves (neither CC cleared the gate; both live in the developer library behind QLINEAR_ONETILE_KC), else CC.

Every case runs its calls twice in one process - default dispatch, then QLINEAR_DISPATCH=noonetile - and wants equal bits.  The counter
qlinear_w4g32_onetile_kc_launches says which kernel served: one per call where the geometry is on, none otherwise, none under noonetile;
qlinear_w4g32_onetile_launches counts it like every one-tile kernel.  A narrow shape has 1 - 3 blocks, so it runs ROWS different
activation rows, one launch each, back to back.

Product library, K = 4096 (the only K its dispatch serves with two slices of one tile):
  N=8    two blocks at CC = 1, one at CC = 2
  N=6    CC = 1: a block with two waves on padded columns - they load in full, pass the barrier and store nothing; CC = 2: a wave with one
         live column (element-wise store)
  N=2    waves with no live column, inside the padded quad and past it
  N=1    the odd element-wise store
  N=12   residual row (and, through the C entry point, output row) at a pointer that is 2-byte but not 4-byte aligned
Developer library (the switch is read once per process: one child process per CC), QLINEAR_W4_KSPLIT=2:
  K=2112  66 groups, 33 per slice: masked lanes in both halves          K=4064  127 groups: one masked lane, in slice 1 only
  N=8 and N=6 each; then every K = 4096 case above for the CC that the product library does not ship.  A third child with
  QLINEAR_ONETILE_KC=0 runs the K = 4096 cases on the lean two-column kernel with the quad combine, which the developer library keeps as
  the baseline of the measurement and which no default dispatch reaches at two slices any more.
"""
import functools
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from chatglm_q_amd import _lib  # noqa: E402
from chatglm_q_amd.int4 import hip_ops as h4  # noqa: E402

PRODUCT_KC = 1
DEV = "cuda:0"
TDT = {"f16": torch.float16, "bf16": torch.bfloat16}
SHAPES = [(4096, 8), (4096, 6), (4096, 2), (4096, 1)]
DEV_SHAPES = [(2112, 8), (2112, 6), (4064, 8), (4064, 6)]
ENTRIES = ["plain", "bias", "residual", "residual_bias"]
ROWS = 32


@functools.lru_cache(maxsize=None)
def weights(K, N, dt):
    g = torch.Generator().manual_seed(K * 7 + N)
    qd = torch.randint(0, 256, (K // 2, N), dtype=torch.uint8, generator=g).to(DEV)
    sd = (torch.rand((K // 32, N), generator=g) * 0.02 + 0.002).to(TDT[dt]).to(DEV)
    bias = (torch.randn(N, generator=g) * 0.1).to(TDT[dt]).to(DEV)
    return qd, sd, h4.repack_w4g32(qd, sd), bias


@pytest.fixture(autouse=True)
def dispatch_as_the_environment_says():
    """After every test the library's parsed flags follow QLINEAR_DISPATCH as the environment has it (both_kernels changes and restores it)."""
    yield
    _lib.get_lib().qlinear_dispatch_reload()


def counters():
    lib = _lib.get_lib()
    return int(lib.qlinear_w4g32_onetile_launches()), int(lib.qlinear_w4g32_onetile_kc_launches())


def both_kernels(call, calls, kc_on):
    """call() under the default dispatch and under noonetile.  Both counters are checked: the one-tile counter advances by one per call, the
    K-complete counter with it where the geometry is on and not at all where it is off; neither moves under noonetile."""
    lib = _lib.get_lib()
    os.environ.pop("QLINEAR_DISPATCH", None)
    lib.qlinear_dispatch_reload()
    n0 = counters()
    new = call()
    n1 = counters()
    try:
        os.environ["QLINEAR_DISPATCH"] = "noonetile"
        lib.qlinear_dispatch_reload()
        assert lib.qlinear_dispatch_flags() & 256
        old = call()
        n2 = counters()
    finally:
        os.environ.pop("QLINEAR_DISPATCH", None)
        lib.qlinear_dispatch_reload()
    torch.cuda.synchronize()
    assert n1[0] - n0[0] == calls, "the default dispatch did not take a one-tile kernel once per call"
    assert n1[1] - n0[1] == (calls if kc_on else 0), ("K-complete launches", n1[1] - n0[1], calls, kc_on)
    assert n2 == n1, "noonetile still launched a one-tile kernel"
    return new, old


def entry_call(entry, K, N, dt, strict, row):
    qd, sd, packed, bias = weights(K, N, dt)
    g = torch.Generator().manual_seed(3 * K + N + 17 * len(entry) + 1000 * row)
    a = torch.randn((1, 1, K), generator=g).to(TDT[dt]).to(DEV)
    bd = bias if entry in ("bias", "residual_bias") else None
    if entry in ("plain", "bias"):
        return lambda: h4.w4_forward(a.reshape(1, K), qd, sd, bd, packed, strict=strict)
    res = torch.randn((1, 1, N), generator=g).to(TDT[dt]).to(DEV)
    return lambda: h4.w4_forward_residual(a, packed, N, bd, res, strict=strict)


def case_equals_tile_loop(K, N, entry, dt, strict, kc_on):
    calls = [entry_call(entry, K, N, dt, strict, r) for r in range(ROWS)]
    new, old = both_kernels(lambda: [c() for c in calls], ROWS, kc_on)              # ROWS launches back to back, no sync between them
    for r, (x, y) in enumerate(zip(new, old)):
        assert x.shape[-1] == N and torch.equal(x, y), (K, N, entry, dt, strict, r, (x != y).sum().item())
    assert len({tuple(x.flatten().tolist()) for x in new}) > 1, "32 different rows gave one result: the comparison would be vacuous"


def odd_pointers_equal_tile_loop(entry, dt, strict, kc_on):
    """K=4096 N=12.  The residual row is a [1:] slice of a longer tensor, so its pointer is 2-byte but not 4-byte aligned; the entry point
    accepts that today (the tile-loop kernel then reads element-wise).  Then the same call through the C entry point with the OUTPUT row
    at such a pointer as well: no 4-byte store may be taken for it."""
    K, N = 4096, 12
    qd, sd, packed, bias = weights(K, N, dt)
    bd = bias if entry == "residual_bias" else None
    g = torch.Generator().manual_seed(99 + len(entry))
    rows = [torch.randn((1, 1, K), generator=g).to(TDT[dt]).to(DEV) for _ in range(ROWS)]
    longer = torch.randn(N + 1, generator=g).to(TDT[dt]).to(DEV)
    res = longer[1:]
    assert res.data_ptr() % 4 == 2 and res.is_contiguous()
    new, old = both_kernels(lambda: [h4.w4_forward_residual(a, packed, N, bd, res, strict=strict) for a in rows], ROWS, kc_on)
    for r, (x, y) in enumerate(zip(new, old)):
        assert torch.equal(x, y), (entry, dt, strict, r, (x != y).sum().item())
    assert len({tuple(x.flatten().tolist()) for x in new}) > 1

    lib = _lib.get_lib()
    flags = _lib.FLAG_STRICT_ROUNDING if strict else 0

    def into_odd_rows():
        outs = [torch.zeros(N + 3, device=DEV, dtype=TDT[dt]) for _ in rows]
        for a, o in zip(rows, outs):
            assert o[1:].data_ptr() % 4 == 2
            with torch.cuda.device(a.device):
                st = lib.qlinear_w4g32_fwd_packed_residual(a.data_ptr(), packed.data_ptr(), _lib.ptr(bd), res.data_ptr(), o[1:].data_ptr(), N, K,
                                                           _lib.dtype_code(a.dtype), flags, _lib.stream_ptr(a.device))
            _lib.check(st, "qlinear_w4g32_fwd_packed_residual")
        return outs

    new2, old2 = both_kernels(into_odd_rows, ROWS, kc_on)
    for r, (x, y, z) in enumerate(zip(new2, old2, new)):
        assert torch.equal(x, y) and torch.equal(x[1:N + 1], z.flatten()), (entry, dt, strict, r)
        assert x[0].item() == 0 and x[N + 1:].abs().sum().item() == 0, "a store outside the output row"


def graph_replay_equals_eager(kc_on):
    K, N = 4096, 8
    qd, sd, packed, bias = weights(K, N, "f16")
    a = torch.randn((1, K), generator=torch.Generator().manual_seed(5)).half().to(DEV)
    n0 = counters()
    eager = h4.w4_forward(a, qd, sd, bias, packed, strict=False)
    n1 = counters()
    assert n1[0] - n0[0] == 1 and n1[1] - n0[1] == (1 if kc_on else 0)
    stream = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(stream):
        h4.w4_forward(a, qd, sd, bias, packed, strict=False)       # warm-up outside the capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            out = h4.w4_forward(a, qd, sd, bias, packed, strict=False)
        for _ in range(2):
            out.zero_()
            graph.replay()
            stream.synchronize()
            assert torch.equal(out, eager)


@pytest.mark.parametrize("strict", [False, True], ids=["default", "strict"])
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("K,N", SHAPES)
def test_default_dispatch_equals_tile_loop(K, N, entry, dt, strict):
    case_equals_tile_loop(K, N, entry, dt, strict, PRODUCT_KC != 0)


@pytest.mark.parametrize("strict", [False, True], ids=["default", "strict"])
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("entry", ["residual", "residual_bias"])
def test_odd_residual_and_output_pointers(entry, dt, strict):
    odd_pointers_equal_tile_loop(entry, dt, strict, PRODUCT_KC != 0)


def test_graph_replay_equals_eager():
    """(4096, 8) captured once and replayed twice: every replay equals the eager result."""
    graph_replay_equals_eager(PRODUCT_KC != 0)


def test_counter_is_off_where_the_geometry_does_not_apply():
    """One K slice (K = 2048) and the 4-slice shapes keep their kernels: the K-complete counter stays, the one-tile counter advances."""
    call = entry_call("plain", 2048, 8, "f16", False, 0)
    both_kernels(call, 1, False)


def test_geometries_of_the_developer_library_equal_tile_loop():
    """One child process per CC on libqlinear_hip_dev.so, QLINEAR_W4_KSPLIT=2 and QLINEAR_ONETILE_KC=CC: the shapes with masked lanes, and for
    the CC that the product library does not run every K = 4096 case above, the odd pointers and the graph replay."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dev = os.path.join(root, "chatglm_q_amd", "csrc", "libqlinear_hip_dev.so")
    assert os.path.exists(dev), "the developer library is part of build()"
    for cc in (1, 2, 0):
        env = dict(os.environ, QLINEAR_LIB_PATH=dev, QLINEAR_W4_KSPLIT="2", QLINEAR_ONETILE_KC=str(cc), PYTHONPATH=root)
        for name in ("QLINEAR_DISPATCH", "QLINEAR_ONETILE_TICKET", "QLINEAR_ONETILE_LEAN", "QLINEAR_ONETILE_CW"):
            env.pop(name, None)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--kc-child", str(cc)], env=env, capture_output=True, text=True, timeout=120)
        cases = (64 if cc else 0) + (0 if cc == PRODUCT_KC else 64 + 8)
        want = f"kc child ok: CC={cc}, {cases} cases" + ("" if cc == PRODUCT_KC else ", graph replay")
        assert out.returncode == 0 and want in out.stdout, (cc, out.stdout[-2000:], out.stderr[-2000:])


def _kc_child(cc):
    cases = 0
    shapes = (DEV_SHAPES if cc else []) + ([] if cc == PRODUCT_KC else SHAPES)
    for K, N in shapes:
        for entry in ENTRIES:
            for dt in TDT:
                for strict in (False, True):
                    case_equals_tile_loop(K, N, entry, dt, strict, cc != 0)
                    cases += 1
    tail = ""
    if cc != PRODUCT_KC:
        for entry in ("residual", "residual_bias"):
            for dt in TDT:
                for strict in (False, True):
                    odd_pointers_equal_tile_loop(entry, dt, strict, cc != 0)
                    cases += 1
        graph_replay_equals_eager(cc != 0)
        tail = ", graph replay"
    print(f"kc child ok: CC={cc}, {cases} cases{tail}")


if __name__ == "__main__" and "--kc-child" in sys.argv:
    _kc_child(int(sys.argv[sys.argv.index("--kc-child") + 1]))

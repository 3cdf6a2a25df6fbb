"""Entry and exit of the one-tile one-row int4g32 GEMV's plain / residual forward (w4_packed.hip) against the tile-loop kernel, BIT FOR BIT:
LEAN - the body that knows M == 1 and addresses everything by 32-bit byte offsets against scalar bases (the default dispatch) - and
TICKET - the quad's sums meet in LDS through an arrival ticket instead of a barrier hand-over to the quad's first wave (measured slower,
so the developer library only: QLINEAR_ONETILE_TICKET=1; the switch is read once per process, hence one child process for all its cases).

Every case runs its calls twice in one process - default dispatch, then QLINEAR_DISPATCH=noonetile - and wants equal bits; the library's
launch counter of the one-tile kernel says which kernel served each (one per call, none under noonetile).  A narrow shape has 1 - 2
blocks, so it runs ROWS different activation rows, one launch each, back to back: every launch zeroes its tickets anew and the waves of
a quad arrive in whatever order the hardware produces.

Shapes: the smallest that reach each new branch -
  K=4096 N=8   two K slices: four waves per quad, one ticket per block; a block whose spare waves shadow quad 0
  K=4096 N=6   partial quad: element-wise epilogue (with tickets: run by the last arriver)
  K=4096 N=2   a two-column wave with no live column (with tickets: it draws one all the same)
  K=2048 N=8   one slice: two waves per quad, two tickets per block
  K=1056 N=8   33 groups: masked lanes
  K=2048 N=2^21+8   the packed buffer is larger than 2^31 bytes: the lean entry's 32-bit offsets do not apply, the launcher takes the body
                    with 64-bit addresses
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

DEV = "cuda:0"
TDT = {"f16": torch.float16, "bf16": torch.bfloat16}
SHAPES = [(4096, 8), (4096, 6), (4096, 2), (2048, 8), (1056, 8)]
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
    """Set up first, so finalised after monkeypatch has put QLINEAR_DISPATCH back: the library's parsed flags follow the variable again."""
    yield
    _lib.get_lib().qlinear_dispatch_reload()


def onetile_launches():
    return int(_lib.get_lib().qlinear_w4g32_onetile_launches())


def both_kernels(call, monkeypatch, calls):
    """call() under the default dispatch and under noonetile; the counter advances by one per one-tile call and by zero under noonetile."""
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
    assert n1 - n0 == calls, "the default dispatch did not take the one-tile kernel once per call"
    assert n2 - n1 == 0, "noonetile still launched the one-tile kernel"
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


@pytest.mark.parametrize("strict", [False, True], ids=["default", "strict"])
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("K,N", SHAPES)
def test_entry_exit_equals_tile_loop(K, N, entry, dt, strict, monkeypatch):
    calls = [entry_call(entry, K, N, dt, strict, r) for r in range(ROWS)]
    new, old = both_kernels(lambda: [c() for c in calls], monkeypatch, ROWS)     # ROWS launches back to back, no sync between them
    for r, (x, y) in enumerate(zip(new, old)):
        assert x.shape[-1] == N and torch.equal(x, y), (K, N, entry, dt, strict, r, (x != y).sum().item())
    assert len({tuple(x.flatten().tolist()) for x in new}) > 1, "32 different rows gave one result: the comparison would be vacuous"


def test_ticket_combine_of_the_developer_library_equals_tile_loop():
    """Every case above and the graph replay once more in a child process on libqlinear_hip_dev.so with QLINEAR_ONETILE_TICKET=1, with
    and without the lean entry."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dev = os.path.join(root, "chatglm_q_amd", "csrc", "libqlinear_hip_dev.so")
    assert os.path.exists(dev), "the developer library is part of build()"
    for lean in ("1", "0"):
        env = dict(os.environ, QLINEAR_LIB_PATH=dev, QLINEAR_ONETILE_TICKET="1", QLINEAR_ONETILE_LEAN=lean, PYTHONPATH=root)
        env.pop("QLINEAR_DISPATCH", None)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--ticket-child"], env=env, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and "ticket child ok: 80 cases, graph replay" in out.stdout, (lean, out.stdout[-2000:], out.stderr[-2000:])


def _ticket_child():
    lib = _lib.get_lib()
    cases = 0
    for K, N in SHAPES:
        for entry in ENTRIES:
            for dt in TDT:
                for strict in (False, True):
                    calls = [entry_call(entry, K, N, dt, strict, r) for r in range(ROWS)]
                    os.environ.pop("QLINEAR_DISPATCH", None)
                    lib.qlinear_dispatch_reload()
                    n0 = onetile_launches()
                    new = [c() for c in calls]
                    assert onetile_launches() - n0 == ROWS
                    os.environ["QLINEAR_DISPATCH"] = "noonetile"
                    lib.qlinear_dispatch_reload()
                    old = [c() for c in calls]
                    assert onetile_launches() - n0 == ROWS
                    torch.cuda.synchronize()
                    for r, (x, y) in enumerate(zip(new, old)):
                        assert torch.equal(x, y), (K, N, entry, dt, strict, r, (x != y).sum().item())
                    cases += 1
    os.environ.pop("QLINEAR_DISPATCH", None)
    lib.qlinear_dispatch_reload()
    graph_replay_equals_eager()            # with tickets: every replay zeroes them anew
    print(f"ticket child ok: {cases} cases, graph replay")


def test_offsets_past_31_bits_take_the_64_bit_body(monkeypatch):
    """Packed weights of 2^31 + 8192 bytes: byte offsets no longer fit 31 bits, so the plain forward runs the one-tile body with 64-bit
    addresses.  Every output, the last columns (whose weight words lie past 2^31) included, equals the tile-loop kernel's."""
    K, N = 2048, (1 << 21) + 8
    g = torch.Generator(device=DEV).manual_seed(11)
    qd = torch.randint(0, 256, (K // 2, N), dtype=torch.uint8, device=DEV, generator=g)
    sd = (torch.rand((K // 32, N), device=DEV, generator=g) * 0.02 + 0.002).half()
    packed = h4.repack_w4g32_gemv(qd, sd)                          # part 1 alone: what one row reads
    assert packed.numel() > (1 << 31)
    a = torch.randn((1, K), device=DEV, generator=g).half()
    new, old = both_kernels(lambda: h4.w4_forward(a, qd, sd, None, packed, strict=False), monkeypatch, 1)
    assert torch.equal(new, old), (new != old).sum().item()
    assert new[0, -8:].float().abs().sum().item() > 0
    del qd, sd, packed
    torch.cuda.empty_cache()


def test_counter_follows_the_dispatch(monkeypatch):
    """qlinear_w4g32_onetile_launches: +1 per one-tile call on the new paths exactly as on the kernel they replace, +0 under noonetile."""
    call = entry_call("plain", 4096, 8, "f16", False, 0)
    lib = _lib.get_lib()
    lib.qlinear_dispatch_reload()
    n0 = onetile_launches()
    for i in range(1, 4):
        call()
        assert onetile_launches() - n0 == i
    both_kernels(call, monkeypatch, 1)


def test_graph_replay_equals_eager():
    """(4096, 8) captured once and replayed three times: every replay equals the eager result (the lean entry here; the ticket combine's
    replay runs in the developer library's child process above)."""
    graph_replay_equals_eager()


def graph_replay_equals_eager():
    K, N = 4096, 8
    qd, sd, packed, bias = weights(K, N, "f16")
    a = torch.randn((1, K), generator=torch.Generator().manual_seed(5)).half().to(DEV)
    n0 = onetile_launches()
    eager = h4.w4_forward(a, qd, sd, bias, packed, strict=False)
    assert onetile_launches() - n0 == 1
    stream = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(stream):
        h4.w4_forward(a, qd, sd, bias, packed, strict=False)       # warm-up outside the capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            out = h4.w4_forward(a, qd, sd, bias, packed, strict=False)
        for _ in range(3):
            out.zero_()
            graph.replay()
            stream.synchronize()
            assert torch.equal(out, eager)


if __name__ == "__main__" and "--ticket-child" in sys.argv:
    _ticket_child()

"""GPTQ on the GPU: ``qlinear_gptq_block`` (csrc/gptq.hip) through ``fused_ops.gptq_block`` against the numpy oracle
(tests/_gptq_oracle.py) BIT FOR BIT - every operation of the walk is a single correctly rounded fp32 operation, so exact equality is
asked -, against the reference's recorded results (tests/golden/gptq.npz), and ``GPTQLinearQuantizer.quantize_weight`` /
``gptq_quantize_model_`` end to end under the row conditions of tests/test_gptq_cpu.py."""
import numpy as np
import pytest
import torch

import _gptq_oracle as GO
from chatglm_q_amd import _gptq_core, _lib, fused_ops
from chatglm_q_amd.gptq import gptq_quantize_model_
from test_gptq_cpu import MODS, armed_quantizer, check_end_to_end, fixture, rtn_error, tiny_batches, tiny_float_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32


def random_factor(rs, n, dead=None):
    """An upper-triangular (n, n) fp32 matrix with a positive diagonal - the shape of the factor, no more is needed to pin the
    arithmetic.  ``dead``: a column whose row and column hold only the diagonal, as a dead input feature's do."""
    h = np.triu(rs.standard_normal((n, n)) * 0.05, 1).astype(F32)
    h[np.diag_indices(n)] = (0.5 + rs.random_sample(n)).astype(F32)
    if dead is not None:
        h[dead, dead + 1:] = 0
        h[:dead, dead] = 0
    return h


def run_both(W, c0, bc, hinv, bits, scale_np):
    """The kernel and the oracle on the same block; returns ((Q, Err, Loss, scale) of each)."""
    s_o = scale_np.copy()
    want = GO.gptq_block(W, c0, bc, hinv, bits, s_o)
    Wd, s_d = torch.from_numpy(W).to(DEV), torch.from_numpy(scale_np.copy()).to(DEV)
    keep = Wd.clone()
    got = fused_ops.gptq_block(Wd, c0, bc, torch.from_numpy(hinv).to(DEV), bits, s_d)
    torch.cuda.synchronize()
    assert torch.equal(Wd, keep)                                 # the weights are read only
    return want + (s_o,), tuple(t.cpu().numpy() for t in got) + (s_d.cpu().numpy(),)


def assert_bits(want, got):
    for name, w, g in zip(("Q", "Err", "Loss", "scale"), want, got):
        same = w.view(np.int32) == g.view(np.int32)
        assert same.all(), f"{name}: {int((~same).sum())} of {same.size} elements differ, first at {np.argwhere(~same)[0]}"


def block_case(rows, bc, bits, c0, extra, seed, dead=True):
    rs = np.random.RandomState(seed)
    C = c0 + bc + extra
    W = (rs.standard_normal((rows, C)) * 0.05).astype(F32)
    dcol = c0 + bc // 2 if dead and bc > 2 else None
    if dcol is not None:
        W[:, dcol] = 0
    hinv = random_factor(rs, C, dcol)
    if bits == 4:
        scale = np.full((C // 32, rows), -1.0, dtype=F32)        # sentinel: only the block's rows may change
    else:
        scale = np.maximum(np.abs(W).max(axis=1) / F32(127), F32(1e-10))
    return W, hinv, scale


@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("bc", [32, 64, 128])
@pytest.mark.parametrize("rows", [1, 63, 96, 4096, 65024])
def test_kernel_equals_oracle(rows, bc, bits):
    c0, extra = 64, 32                                           # c0 > 0 and ldw > bc: the block sits inside a wider matrix
    W, hinv, scale = block_case(rows, bc, bits, c0, extra, 100 * bc + bits + rows % 97)
    want, got = run_both(W, c0, bc, hinv, bits, scale)
    assert_bits(want, got)
    if bits == 4:
        untouched = np.ones(scale.shape[0], dtype=bool)
        untouched[c0 // 32:(c0 + bc) // 32] = False
        assert (got[3][untouched] == -1.0).all() and (got[3][~untouched] > 0).all()


@pytest.mark.parametrize("bc,c0", [(1, 0), (2, 7), (31, 3), (33, 32), (37, 5), (100, 1), (127, 0), (128, 1)])
def test_kernel_int8_ragged_blocks(bc, c0):
    # int8 takes any width: whole 32-column chunks in registers, the ragged end through its own loop; unaligned first column
    W, hinv, scale = block_case(130, bc, 8, c0, 3, 900 + bc)
    assert_bits(*run_both(W, c0, bc, hinv, 8, scale))


@pytest.mark.parametrize("bits", [4, 8])
def test_kernel_value_edges(bits):
    """Rows built so that the walk meets: an all-zero row (the int4 scale clamps to 1e-10), exact half ties w / s = k + 0.5 (round
    half to even), values that saturate at +-qmax, a dead column.  A diagonal factor keeps every column as it was set; the same
    rows then run under a full factor, where column 0 still holds what was set."""
    qmax = 7 if bits == 4 else 127
    rows, bc = 70, 64
    rs = np.random.RandomState(4242 + bits)
    s0 = F32(2.0 ** -5)                                          # a power of two: (k + 0.5) * s0 and 7 * s0 are exact
    W = np.zeros((rows, bc), dtype=F32)
    k = rs.randint(-qmax, qmax, size=(rows, bc)).astype(F32)
    W[:] = (k + F32(0.5)) * s0                                   # every entry an exact tie
    W[:, 0::32] = F32(qmax) * s0                                 # int4: pins each group's maximum, so its scale is s0
    W[1] = 0                                                     # all-zero row
    W[2, 1::2] = F32(3 * qmax) * s0                              # int8: far beyond the scale -> saturates at +qmax
    W[3, 1::2] = -F32(3 * qmax) * s0
    W[:, 40] = 0                                                 # dead column
    if bits == 4:
        W[2:4] = np.clip(W[2:4], -F32(qmax) * s0, F32(qmax) * s0)   # int4 takes its scale from the row: saturation comes below
        scale = np.zeros((bc // 32, rows), dtype=F32)
    else:
        scale = np.full(rows, s0, dtype=F32)
        scale[1] = F32(1e-10)
    diag = np.diag((0.5 + rs.random_sample(bc)).astype(F32)).astype(F32)
    want, got = run_both(W, 0, bc, diag, bits, scale)
    assert_bits(want, got)
    x = W[0] / s0
    tie = (x - np.floor(x)) == 0.5
    assert tie.sum() >= bc - 4 and (np.rint(got[0][0] / s0)[tie] % 2 == 0).all()
    assert not got[0][1].any() and not got[1][1].any()           # the zero row stays zero, no NaN from 0 / 1e-10
    if bits == 4:
        assert (got[3][:, 1] == F32(1e-10)).all()
    else:
        assert (got[0][2, 1::2] == F32(qmax) * s0).all() and (got[0][3, 1::2] == -F32(qmax) * s0).all()
    full = random_factor(rs, bc, 40)
    full[1, 2:] *= F32(40)                  # column 1 is a tie, so its error is half a step: a strong row 1 pushes the columns after it
    want, got = run_both(W, 0, bc, full, bits, scale)
    assert_bits(want, got)
    if bits == 4:                           # ... past the maximum the group's scale was taken from: |w - q| beyond half a step = saturated
        e = np.abs(got[1] * np.diag(full)[None, :])
        assert (e[:, :32] > F32(0.51) * got[3][0][:, None]).sum() > 10


@pytest.mark.parametrize("bits", ["int4", "int8"])
def test_kernel_equals_reference_on_fixture_a(bits):
    fx = fixture("a", bits)
    nbits = MODS[bits][1]
    W = fx["W"].copy()
    scale = (np.zeros((4, 96), dtype=F32) if nbits == 4
             else np.maximum(np.abs(W).max(axis=1) / F32(127), F32(1e-10)))      # int8: from the ORIGINAL weights
    W[:, GO.CASES["a"][2]] = 0
    _, got = run_both(W, 0, 128, fx["hinv"], nbits, scale)
    assert np.array_equal(got[0].view(np.int32), fx["grid"].view(np.int32))
    assert np.array_equal(got[3].view(np.int32), fx["scale"].view(np.int32))


@pytest.mark.parametrize("bits", ["int4", "int8"])
@pytest.mark.parametrize("name", ["a", "b"])
def test_quantize_weight_end_to_end(name, bits):
    q, fx = armed_quantizer(name, bits, DEV)
    before = _lib.launch_count()
    grid, scale, quant_losses, debug_loss = q.quantize_weight()          # a contiguous fp32 weight on the GPU: the kernel
    n_blocks = -(-fx["W"].shape[1] // 128)
    assert _lib.launch_count() - before == n_blocks
    kernel = (grid.cpu().numpy(), scale.cpu().numpy(), quant_losses, debug_loss)
    check_end_to_end(*kernel, fx, bits, label=f"kernel {name}/")
    assert GO.hessian_error(fx["W"], kernel[0], fx["hessian"]) < rtn_error(fx, bits)
    # the composed path on the same GPU: no launch through the library, the same result by rows
    q2, _ = armed_quantizer(name, bits, DEV)
    before = _lib.launch_count()
    grid2, scale2, ql2, dl2 = q2.quantize_weight(use_kernel=False)
    assert _lib.launch_count() == before
    check_end_to_end(*kernel, fx, bits, other=(grid2.cpu().numpy(), scale2.cpu().numpy(), ql2, dl2), label=f"kernel vs composed {name}/")
    check_end_to_end(grid2.cpu().numpy(), scale2.cpu().numpy(), ql2, dl2, fx, bits, label=f"composed {name}/")


@pytest.mark.parametrize("bits", ["int4", "int8"])
def test_launch_accounting(bits):
    for blocksize, want in ((128, 3), (64, 5), (96, 4)):
        if bits == "int4" and blocksize % 32:
            continue
        q, _ = armed_quantizer("b", bits, DEV)
        before = _lib.launch_count()
        q.quantize_weight(blocksize=blocksize, use_kernel=True)
        assert _lib.launch_count() - before == want == -(-320 // blocksize)
    q, _ = armed_quantizer("b", bits, DEV)
    new = q.get_quantized_linear()
    assert new.weight.device.type == "cuda" and new.weight_scale.device.type == "cuda"


@pytest.mark.parametrize("quant_type", ["int4g32", "int8"])
def test_driver_kernel_against_composed(quant_type, monkeypatch):
    models = {}
    for use_kernel in (True, False):
        monkeypatch.setattr(_gptq_core, "USE_KERNEL", use_kernel)
        m = tiny_float_model()
        before = _lib.launch_count()
        gptq_quantize_model_(m, tiny_batches(), quant_type, device=DEV)
        launched = _lib.launch_count() - before
        assert next(m.parameters()).device.type == "cpu"          # every layer went to the GPU and came back
        models[use_kernel] = {k: v.cpu() for k, v in m.state_dict().items()}
        if use_kernel:
            assert launched >= 9                                  # one block launch per linear at least (all are <= 128 columns wide)
    a, b = models[True], models[False]
    for key in a:
        if not key.endswith(".weight") or key.startswith("word_embedding") or a[key].dtype not in (torch.uint8, torch.int8):
            continue
        sk = key + "_scale"
        if quant_type == "int4g32":                               # (K / 2, N) packed, (K / 32, N) scales: a linear's row is a column here
            differs = (a[key] != b[key]).any(dim=0)
            sa, sb = a[sk].t(), b[sk].t()
        else:
            differs = (a[key] != b[key]).any(dim=1)
            sa, sb = a[sk][:, None], b[sk][:, None]
        n = differs.numel()
        print(f"{quant_type} {key}: rows differing {int(differs.sum())} of {n}")
        assert int(differs.sum()) <= max(1, n // 100), key
        ok = ~differs
        assert float(((sa[ok] - sb[ok]).abs() / sb[ok]).max()) <= 1e-5, key


def test_status_codes():
    lib = _lib.get_lib()
    rows, C = 8, 160
    W = torch.zeros(rows, C, device=DEV)
    H = torch.eye(C, device=DEV)
    Q, E, L = (torch.empty(rows, 128, device=DEV) for _ in range(3))
    s4, s8 = torch.zeros(C // 32, rows, device=DEV), torch.ones(rows, device=DEV)
    st = _lib.stream_ptr(torch.device(DEV))

    def call(W=W.data_ptr(), n_rows=rows, ldw=C, c0=0, bc=128, H=H.data_ptr(), ldh=C, bits=4, group=32, Q=Q.data_ptr(), E=E.data_ptr(),
             L=L.data_ptr(), scale=None, lds=rows, dtype=0):
        scale = (s4 if bits == 4 else s8).data_ptr() if scale is None else scale
        return lib.qlinear_gptq_block(W, n_rows, ldw, c0, bc, H, ldh, bits, group, Q, E, L, scale, lds, dtype, st)

    NULL, SHAPE, DTYPE, UNSUP = -1, -2, -3, _lib.ERR_UNSUPPORTED
    before = _lib.launch_count()
    assert call(dtype=1) == DTYPE and call(dtype=2) == DTYPE and call(dtype=7) == DTYPE
    assert call(bits=3) == UNSUP and call(bits=16) == UNSUP
    assert call(group=64) == UNSUP and call(group=16) == UNSUP and call(group=0) == UNSUP
    assert call(bc=0) == SHAPE and call(bc=129) == SHAPE and call(bits=8, bc=129) == SHAPE
    assert call(bc=48) == SHAPE and call(c0=16, bc=32) == SHAPE           # int4: whole groups only
    assert call(c0=64) == SHAPE                                          # c0 + bc > ldw
    assert call(ldh=127) == SHAPE and call(n_rows=-1) == SHAPE and call(lds=rows - 1) == SHAPE
    for null in ("W", "H", "Q", "E", "L"):
        assert call(**{null: 0}) == NULL
    assert call(scale=0) == NULL and call(bits=8, scale=0) == NULL
    assert call(n_rows=0) == 0 and call(n_rows=0, W=0) == 0              # nothing to do: QL_OK without a launch
    assert _lib.launch_count() == before
    assert call() == 0 and call(bits=8, bc=37, c0=3, group=0) == 0
    torch.cuda.synchronize()
    assert _lib.launch_count() == before + 2
    with pytest.raises(ValueError):
        fused_ops.gptq_block(W, 0, 129, H, 8, s8)
    with pytest.raises(ValueError):
        fused_ops.gptq_block(W.half(), 0, 128, H, 8, s8)
    with pytest.raises(ValueError):
        fused_ops.gptq_block(W, 0, 48, H, 4, s4)

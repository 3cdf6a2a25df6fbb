"""numpy fp32 restatement of GPTQ as this package computes it (include/qlinear_hip.h: qlinear_gptq_block), for the tests.

``gptq_block`` is the contract of the kernel: per weight row, every line ONE fp32 operation rounded to nearest (numpy float32
array arithmetic does not fuse), w[] the row's current block values, d = hinv[j][j], qmax = 7 / 127:

    int4, j % group == 0:  m = max_{t<group} |w[j+t]|;  s = max(m / 7, 1e-10);  scale[(c0+j)/group][r] = s
    int8:                  s = scale[r]
    x = w[j] / s;  c = min(max(rint(x), -qmax), qmax);  q = s * c                    Q[r][j] = q
    e = w[j] - q;  Loss[r][j] = ((e * e) / (d * d)) * 0.5;  err = e / d              Err[r][j] = err
    for t in j+1 .. bc-1:  p = err * hinv[j][t];  w[t] = w[t] - p

``quantize_weight`` is the whole layer: dead columns, damping, the factor (given, or from an fp64 pipeline), the blocks and the
update of the columns right of each block.  ``calibration_inputs`` is the seeded input generator that the fixture
(tests/golden/make_golden_gptq.py -> tests/golden/gptq.npz) and the tests share, so the fixture need not store the inputs.
"""
import numpy as np

F32 = np.float32

# fixture cases: name -> (n_rows, n_columns, dead column, input batches as leading shapes, seed)
CASES = {
    "a": (96, 128, 37, ((2, 60), (128,), (8,)), 7101),        # one block
    "b": (64, 320, 200, ((3, 100), (332,), (8,)), 7102),      # three blocks, the last one 64 wide
}


def calibration_inputs(name):
    """The case's weight (n_rows, n_columns) and its list of input batches (..., n_columns), fp32: correlated inputs (16 latent
    directions + noise), one always-zero feature.  numpy's legacy MT19937 stream: the same bits on every machine."""
    n_rows, n_cols, dead, batches, seed = CASES[name]
    rs = np.random.RandomState(seed)
    W = (rs.standard_normal((n_rows, n_cols)) * 0.05).astype(F32)
    mix = rs.standard_normal((16, n_cols)).astype(F32)
    out = []
    for lead in batches:
        n = int(np.prod(lead))
        x = rs.standard_normal((n, 16)).astype(F32) @ mix * F32(0.25) + rs.standard_normal((n, n_cols)).astype(F32) * F32(0.5)
        x[:, dead] = 0
        out.append(np.ascontiguousarray(x.reshape(*lead, n_cols).astype(F32)))
    return W, out


def unpack_upper(packed, n):
    """(n, n) upper-triangular matrix from its row-major packed upper triangle."""
    m = np.zeros((n, n), dtype=packed.dtype)
    m[np.triu_indices(n)] = packed
    return m


def unpack_symmetric(packed, n):
    m = unpack_upper(packed, n)
    return m + np.triu(m, 1).T


def gptq_block(W, c0, bc, hinv, bits, scale, group=32):
    """Columns [c0, c0 + bc) of W (n_rows, n_columns) fp32.  Returns (Q, Err, Loss), each (n_rows, bc) fp32; int4 writes rows
    c0 / group ... of ``scale`` (n_columns / group, n_rows), int8 reads ``scale`` (n_rows).  W is not modified."""
    assert W.dtype == F32 and hinv.dtype == F32 and scale.dtype == F32 and bits in (4, 8)
    qmax = F32(7 if bits == 4 else 127)
    w = np.array(W[:, c0:c0 + bc], dtype=F32, order="F")          # a column is contiguous
    h = np.ascontiguousarray(hinv[c0:c0 + bc, c0:c0 + bc])
    n_rows = w.shape[0]
    Q, Err, Loss = (np.empty((n_rows, bc), dtype=F32) for _ in range(3))
    tmp = np.empty((n_rows, bc), dtype=F32, order="F")
    s = scale if bits == 8 else None
    for j in range(bc):
        if bits == 4 and j % group == 0:
            m = np.abs(w[:, j:j + group]).max(axis=1)
            s = np.maximum(m / F32(7), F32(1e-10))
            scale[(c0 + j) // group, :] = s
        d = h[j, j]
        col = w[:, j]
        c = np.minimum(np.maximum(np.rint(col / s), -qmax), qmax)
        q = s * c
        e = col - q
        err = e / d
        Q[:, j], Err[:, j], Loss[:, j] = q, err, ((e * e) / (d * d)) * F32(0.5)
        if j + 1 < bc:
            t = tmp[:, j + 1:]
            np.multiply(err[:, None], h[j, j + 1:][None, :], out=t)
            np.subtract(w[:, j + 1:], t, out=w[:, j + 1:])
    assert Q.dtype == F32 and Err.dtype == F32 and Loss.dtype == F32
    return Q, Err, Loss


def factor_fp64(hessian, percdamp=0.01):
    """Damped Hessian -> upper Cholesky factor of its inverse through fp64 (the dead columns already set to 1), as fp32."""
    H = hessian.astype(np.float64)
    H[np.diag_indices_from(H)] += percdamp * np.mean(np.diag(hessian).astype(F32), dtype=F32)
    inv = np.linalg.inv(H)
    inv = (inv + inv.T) * 0.5
    return np.ascontiguousarray(np.linalg.cholesky(inv).T).astype(F32)


def quantize_weight(W, hessian, bits, blocksize=128, group=32, percdamp=0.01, hinv=None):
    """The whole layer.  Returns (grid_weight, scale, quant_losses, hinv): scale (n_columns / group, n_rows) for int4, (n_rows)
    for int8 (from the ORIGINAL weights)."""
    W = np.array(W, dtype=F32)
    n_rows, n_cols = W.shape
    hessian = np.array(hessian, dtype=F32)
    if bits == 8:
        scale = np.maximum(np.abs(W).max(axis=1) / F32(127), F32(1e-10))
    else:
        scale = np.zeros((n_cols // group, n_rows), dtype=F32)
    dead = np.diag(hessian) == 0
    hessian[dead, dead] = 1
    W[:, dead] = 0
    if hinv is None:
        hinv = factor_fp64(hessian, percdamp)
    grid = np.empty_like(W)
    loss = 0.0
    for i1 in range(0, n_cols, blocksize):
        i2 = min(i1 + blocksize, n_cols)
        Q, Err, Loss = gptq_block(W, i1, i2 - i1, hinv, bits, scale, group)
        grid[:, i1:i2] = Q
        loss += float(Loss.sum(dtype=np.float64))
        if i2 < n_cols:
            W[:, i2:] -= Err @ hinv[i1:i2, i2:]
    return grid, scale, loss / W.size, hinv


def codes(grid, scale, bits, group=32):
    """Integer codes (n_rows, n_columns) of a grid weight under its scales."""
    if bits == 8:
        return np.rint(grid / scale[:, None]).astype(np.int32)
    s = np.repeat(scale.T, group, axis=1)                           # (n_rows, n_columns)
    return np.rint(grid / s).astype(np.int32)


def hessian_error(W, Q, hessian):
    """tr((W - Q) H (W - Q)^T) in fp64: what GPTQ minimises."""
    D = (W.astype(np.float64) - Q.astype(np.float64))
    return float(np.einsum("ri,ij,rj->", D, hessian.astype(np.float64), D))

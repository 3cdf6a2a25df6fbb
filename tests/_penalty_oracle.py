"""numpy restatement of the sampling controls' rules (repetition / presence / frequency penalty, logit bias), op for op in
``np.float32`` and ending in ONE cast to the logits dtype.  Written from the specification, not from the kernel:

    state per row: P[v] (v is one of the row's real prompt ids), G[v] (how often the row has generated v so far)
    for every v, x = float32(logit[v]), every line one correctly rounded fp32 operation, no fused multiply-add:
      1. P[v] or G[v] > 0 :  x = x / r if x > 0 else x * r          (a NaN takes the multiply branch and stays NaN)
      2. G[v] > 0         :  m = f * float32(G[v]);  x = x - m;  x = x - p
      3. v has a bias     :  x = x + bias[v]
    the result is rounded once to the logits dtype (nearest even); an entry no rule touches keeps its bits.

Logits travel in their native representation: ``np.float32`` / ``np.float16`` arrays, bf16 as ``np.uint16`` bit patterns (numpy has
no bf16).  ``History`` carries P and G of one row the way a generation advances them."""
import numpy as np
import torch

DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def to_native(t: torch.Tensor) -> np.ndarray:
    """A torch tensor's values in the oracle's representation (bf16: the uint16 bit patterns)."""
    t = t.detach().cpu().contiguous()
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).numpy().view(np.uint16).copy()
    return t.numpy().copy()


def from_native(a: np.ndarray, dt: str) -> torch.Tensor:
    if dt == "bf16":
        return torch.from_numpy(a.view(np.int16).copy()).view(torch.bfloat16)
    return torch.from_numpy(a.copy())


def widen(a: np.ndarray, dt: str) -> np.ndarray:
    if dt == "bf16":
        return (a.astype(np.uint32) << 16).view(np.float32)
    return a.astype(np.float32)


def narrow(x: np.ndarray, dt: str) -> np.ndarray:
    """float32 -> the logits dtype, round to nearest even."""
    x = np.asarray(x, dtype=np.float32)
    if dt == "f32":
        return x.copy()
    if dt == "f16":
        with np.errstate(over="ignore"):
            return x.astype(np.float16)
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(np.isnan(x), ((u >> 16) | 0x40).astype(np.uint16), r)        # a NaN stays a (quiet) NaN


def bits(a: np.ndarray) -> np.ndarray:
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def same(a: np.ndarray, b: np.ndarray, dt: str) -> np.ndarray:
    """Elementwise: equal bit patterns, or both NaN (a NaN's payload is not part of the contract)."""
    na, nb = np.isnan(widen(a, dt)), np.isnan(widen(b, dt))
    return (bits(a) == bits(b)) | (na & nb)


def penalize(logits: np.ndarray, dt: str, P: np.ndarray, G: np.ndarray, r=1.0, p=0.0, f=0.0, bias=None) -> np.ndarray:
    """One row: logits (N,) native, P (N,) bool, G (N,) integer counts, bias {id: value} or None.  Returns the adjusted row, native."""
    x = widen(logits, dt)
    r, p, f = np.float32(r), np.float32(p), np.float32(f)
    y = x.copy()
    seen = P | (G > 0)
    with np.errstate(all="ignore"):
        pos = x > 0                                              # False for a NaN: the multiply branch
        a, m = seen & pos, seen & ~pos
        y[a] = x[a] / r
        y[m] = x[m] * r
        c = G > 0
        t = f * G[c].astype(np.float32)
        y[c] = y[c] - t
        y[c] = y[c] - p
        touched = seen.copy()
        for i, v in (bias or {}).items():
            y[i] = y[i] + np.float32(v)
            touched[i] = True
    out = logits.copy()
    out[touched] = narrow(y[touched], dt)
    return out


class History:
    """P and G of one row: the real prompt ids, and the tokens generated so far as ``count`` is told them."""

    def __init__(self, prompt, N: int):
        self.P = np.zeros(N, dtype=bool)
        self.P[np.asarray(list(prompt), dtype=np.int64)] = True
        self.G = np.zeros(N, dtype=np.int64)

    def count(self, tok: int):
        self.G[int(tok)] += 1
        return self


def argmax_low(row: np.ndarray, dt: str) -> int:
    """Lowest index of the largest value."""
    return int(np.argmax(widen(row, dt)))

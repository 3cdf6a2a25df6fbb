#!/usr/bin/env python3
"""Generate tests/golden/gptq.npz from the REFERENCE's GPTQ quantizers (chatglm_q/int4/quantizer.py:78-196,
chatglm_q/int8/quantizer.py:55-164).

Like the other make_golden*.py scripts this one imports the reference from its read-only checkout, feeds it seeded inputs and
stores data only.  Per case of tests/_gptq_oracle.py::CASES ("a": 96 x 128, one block; "b": 64 x 320, three blocks with a short
last one; both with an always-zero input feature and correlated inputs) an ``nn.Linear`` with the case's weight is run over the
case's input batches under the reference's forward hook, then ``quantize_weight()`` runs with ``torch.linalg.cholesky`` wrapped
so that the factor the reference walks with - the second, ``upper=True`` call - is recorded.  Stored:

    <case>/W                       the weight (n_rows, n_columns)
    <case>/hessian_packed          upper triangle (row-major) of the accumulated Hessian BEFORE quantize_weight touches it
    <case>/n_samples
    <case>/debug_input             the last batch the hook saw (8 rows)
    <case>/hessian_inv_packed      upper triangle of the recorded factor (the same for int4 and int8: checked)
    <case>/<int4|int8>/grid_weight, scale, quant_losses, debug_loss      what the reference returned

The inputs themselves are not stored: tests/_gptq_oracle.py::calibration_inputs regenerates them.

Usage:  CHATGLM_Q_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_gptq.py
"""
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
REF = os.environ.get("CHATGLM_Q_REFERENCE")
if not REF or not os.path.isdir(os.path.join(REF, "chatglm_q")):
    sys.exit("set CHATGLM_Q_REFERENCE to the reference checkout (the folder that holds chatglm_q/)")
sys.path.insert(0, REF)
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))                        # tests/

import numpy as np  # noqa: E402
import torch  # noqa: E402

import _gptq_oracle as GO  # noqa: E402
from chatglm_q.int4 import quantizer as ref4  # noqa: E402
from chatglm_q.int8 import quantizer as ref8  # noqa: E402


def run(name, mod):
    W, batches = GO.calibration_inputs(name)
    layer = torch.nn.Linear(W.shape[1], W.shape[0], bias=False)
    with torch.no_grad():
        layer.weight.copy_(torch.from_numpy(W))
    q = mod.GPTQLinearQuantizer(layer)
    with torch.no_grad():
        for x in batches:
            layer(torch.from_numpy(x))
    q.remove_hook()
    hessian = q.hessian.clone().numpy()
    factors = []
    real = torch.linalg.cholesky

    def recording(*args, **kwargs):
        out = real(*args, **kwargs)
        if kwargs.get("upper"):
            factors.append(out.clone().numpy())
        return out

    torch.linalg.cholesky = recording
    try:
        grid, scale, quant_losses, debug_loss = q.quantize_weight()
    finally:
        torch.linalg.cholesky = real
    assert len(factors) == 1
    return dict(W=W, hessian=hessian, n_samples=q.n_samples, debug_input=q.debug_input.numpy(), hinv=factors[0],
                grid=grid.numpy(), scale=scale.numpy(), quant_losses=quant_losses, debug_loss=debug_loss)


if __name__ == "__main__":
    torch.set_num_threads(1)
    d = {}
    for name in GO.CASES:
        n = GO.CASES[name][1]
        iu = np.triu_indices(n)
        r4, r8 = run(name, ref4), run(name, ref8)
        assert np.array_equal(r4["hessian"], r8["hessian"]) and np.array_equal(r4["hinv"], r8["hinv"])
        assert np.array_equal(r4["hessian"], r4["hessian"].T), "the packed triangle stands for both halves"
        assert not np.tril(r4["hinv"], -1).any()
        d[f"{name}/W"] = r4["W"]
        d[f"{name}/hessian_packed"] = r4["hessian"][iu]
        d[f"{name}/n_samples"] = np.array(r4["n_samples"], dtype=np.int64)
        d[f"{name}/debug_input"] = r4["debug_input"]
        d[f"{name}/hessian_inv_packed"] = r4["hinv"][iu]
        for bits, r in (("int4", r4), ("int8", r8)):
            d[f"{name}/{bits}/grid_weight"] = r["grid"]
            d[f"{name}/{bits}/scale"] = r["scale"]
            d[f"{name}/{bits}/quant_losses"] = np.array(r["quant_losses"], dtype=np.float64)
            d[f"{name}/{bits}/debug_loss"] = np.array(r["debug_loss"], dtype=np.float64)
            print(name, bits, r["grid"].shape, "quant_losses", r["quant_losses"], "debug_loss", r["debug_loss"])
    path = os.path.join(OUT, "gptq.npz")
    np.savez_compressed(path, **d)
    print("wrote gptq.npz", os.path.getsize(path), "bytes")

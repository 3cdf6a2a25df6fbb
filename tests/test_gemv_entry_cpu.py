"""Static checks on the built library (no GPU) for the one-tile one-row int4g32 GEMV kernels, which tests/test_kernel_entry_cpu.py's symbol
selection does not reach: nothing waits for a scalar load between a wave's first instruction and its first weight load, and the lean
plain / residual kernel - eight arguments, all of them preloaded into SGPRs at wave launch - issues no scalar load at all."""
import pytest

import test_kernel_entry_cpu as E


@pytest.mark.parametrize("pattern,what", [
    (r"w4_packed_gemv_16_onetile_kernelIDF16_Li\dELi\dELb[01]ELi0E", "one-tile forward, 64-bit addresses (plain / residual), f16"),
    (r"w4_packed_gemv_16_onetile_kernelIDF16bLi\dELi\dELb[01]ELi0E", "one-tile forward, 64-bit addresses (plain / residual), bf16"),
    (r"w4_packed_gemv_16_onetile_kernelIDF16_Li\dELi\dELb0ELi[23]E", "one-tile forward with the RMSNorm prologues"),
    (r"w4_packed_gemv_16_onetile_lean_kernelIDF16_", "one-tile forward, lean entry, f16"),
    (r"w4_packed_gemv_16_onetile_lean_kernelIDF16b", "one-tile forward, lean entry, bf16"),
])
def test_no_scalar_load_wait_before_the_first_weight_load(pattern, what, tmp_path):
    kernels = E._disassemble(pattern, tmp_path)
    assert kernels, f"no kernel matches {pattern}: the check would be vacuous"
    for name, lines in kernels.items():
        body = E._body_after_preload_prologue(lines)
        first_nt = next((i for i, op in enumerate(body) if op.startswith("global_load_dwordx4") and " nt" in op), None)
        assert first_nt is not None, f"{what}: no streaming weight load found in {name}"
        pending, stalls = [], []
        for op in body[:first_nt]:
            if op.startswith("s_load") or op.startswith("s_buffer_load"):
                pending.append(op)
            elif op.startswith("s_waitcnt") and "lgkmcnt" in op and pending:
                stalls.append((op, list(pending)))
                pending = []
        assert not stalls, f"{what} ({name}): waits for scalar loads before the first weight load: {stalls}"


def test_the_lean_kernel_issues_no_scalar_load(tmp_path):
    kernels = E._disassemble(r"w4_packed_gemv_16_onetile_lean_kernel", tmp_path)
    assert kernels, "no lean kernel in the library: the check would be vacuous"
    for name, lines in kernels.items():
        body = E._body_after_preload_prologue(lines)
        loads = [op for op in body if op.startswith("s_load") or op.startswith("s_buffer_load")]
        assert not loads, f"{name}: scalar loads behind the preloaded arguments: {loads}"

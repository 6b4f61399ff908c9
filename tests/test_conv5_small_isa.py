"""The small-tile conv5 kernels (csrc/conv5.hip, conv5_small_mfma_kernel) in the shipped code object: the same audit
tests/test_build_flags.py holds the 128 x 256 tile to (tools/isa_audit.py) -- no spills, no compiler-inserted `s_waitcnt vmcnt(0)` in
front of an LDS read (it would make the four-stage ring wait for the prefetch it has just issued)."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "diffpir_amd", "csrc", "libdiffpir_hip.so")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


@pytest.mark.skipif(not (os.path.exists(SO) and os.path.exists(OBJDUMP)), reason="needs the built library and llvm-objdump")
def test_small_tile_kernels_carry_no_compiler_inserted_serialisation():
    spec = importlib.util.spec_from_file_location("isa_audit", os.path.join(ROOT, "tools", "isa_audit.py"))
    ia = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ia)
    seen = 0
    for sym, ins in ia.disassemble(SO).items():
        if "conv5_small_mfma_kernel" not in sym:
            continue
        seen += 1
        r = ia.audit(ins)
        # per wave 2 activation + 1 weight DMA instructions per chunk, issued at four places (three prologue chunks + the loop), x 2 for the
        # two descriptors of a virtual concat
        assert r["lds_dma"] >= 12 and r["scratch"] == 0 and r["vmcnt0_before_ds_read"] == 0, (sym, r)
        assert r["vmcnt0_after_load"] <= 1, (sym, r)                 # the one scalar read of the output scale
    assert seen == 4, seen          # {GroupNorm prologue or not} x {f16x3, f16x1}

"""The shipped conv11 code objects (csrc/conv11.hip): both variants are there, free of spills and of compiler-inserted serialisation in front
of the LDS reads.  The kernel's register allocation is at the limit of two workgroups per CU (profiles/conv11/README.md: 254 / 256 VGPRs), so a
change of the source or of the compiler that brings scratch back must fail here, not show up as a slower forward."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "diffpir_amd", "csrc", "libdiffpir_hip.so")
OBJDUMP = "/opt/rocm/llvm/bin/llvm-objdump"


@pytest.mark.skipif(not (os.path.exists(SO) and os.path.exists(OBJDUMP)), reason="needs the built library and llvm-objdump")
def test_conv11_variants_have_no_scratch_and_no_drained_waits():
    spec = importlib.util.spec_from_file_location("isa_audit", os.path.join(ROOT, "tools", "isa_audit.py"))
    ia = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ia)
    seen = {}
    for sym, ins in ia.disassemble(SO).items():
        if "conv11_mfma_kernel" not in sym:
            continue
        r = ia.audit(ins)
        emit = "ILb1EE" in sym
        seen[emit] = r
        # period bodies: 864 MFMAs each, two slot parities (+ the plain variant's separate last period); the patch pieces of the prologue and
        # of every period body by LDS-DMA
        assert r["mfma"] == (2 * 864 if emit else 3 * 864), (sym, r)
        assert r["scratch"] == 0 and r["vmcnt0_before_ds_read"] == 0 and r["lds_dma"] >= 6, (sym, r)
        # the plane-emitting variant polls its image's arrival counter and reads the group sums back (deliberate load -> wait pairs)
        assert r["vmcnt0_after_load"] <= (6 if emit else 1), (sym, r)
    assert sorted(seen) == [False, True], f"expected the plain and the emitting instantiation, found {sorted(seen)}"

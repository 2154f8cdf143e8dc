"""The four kernels of the strict step get their leading arguments preloaded into SGPRs (gfx950 kernarg preload).

Read from the kernel descriptors of the built library's gfx950 code objects (tools/kernarg_preload.py): a signature that starts with
a by-value struct, or a build without `-mllvm -amdgpu-kernarg-preload-count`, leaves the length at 0 and the wavefronts back on a
scalar-load round in front of their first request.  CPU only: nothing is launched."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernarg_preload as kp      # noqa: E402

STRICT_STEP_KERNELS = ("neg_fwd_edge_kernel", "loss_kernel_reg", "neg_bwd_gemm_kernel", "update_kernel_reg")

pytestmark = pytest.mark.skipif(not os.path.exists(kp.READELF), reason="llvm-readelf of ROCm's LLVM is not installed")


@pytest.fixture(scope="module")
def lengths():
    import __graft_entry__ as entry
    entry.build()
    out = kp.preload_lengths(entry.LIB)
    assert out, "no gfx950 kernel descriptors found in %s" % entry.LIB
    return out


@pytest.mark.parametrize("kernel", STRICT_STEP_KERNELS)
def test_strict_step_kernel_preloads_arguments(lengths, kernel):
    # demangled name prefix `void <kernel><...>(`: every instance of the template, whatever its arguments
    inst = {n: v for n, v in lengths.items() if n.startswith("void %s<" % kernel) or n.startswith("%s(" % kernel)}
    assert inst, "no instance of %s in the library" % kernel
    off = sorted(n for n, v in inst.items() if v == 0)
    assert not off, "kernarg preload length 0: %s" % off
    print("%s: %d instances, preload length %s dwords" % (kernel, len(inst), sorted(set(inst.values()))))

"""ISA check of k_wgrad_mix's LDS-DMA loads (DESIGN.md section 4's operand rule, as for k_wgrad_dma and
k_wgrad_tr): in the instantiation of the gfx950 build the tool finds the pinned loads -- offset VGPRs advanced
in place, the two resources in SGPRs -- and no instruction between a register's first DMA and the loop's last
barrier rewrites one of them (tools/check_wgrad_operands.py; hipcc cross-compiles, no GPU needed)."""
import os
import shutil
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("/opt/rocm/bin/hipcc") is None, reason="hipcc not installed")
def test_wgrad_mix_dma_operands_never_rewritten():
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "check_wgrad_operands.py")],
                       capture_output=True, text=True, timeout=600)
    lines = [l for l in r.stdout.splitlines() if "k_wgrad_mix" in l]
    assert len(lines) == 1, r.stdout + r.stderr  # 264 x 460: 17 x 8 tiles per block
    assert all("foreign writes 0" in l for l in lines), r.stdout
    # two offset sets of 5 (dY) + 2 (X) VGPRs and two 4-SGPR resources: the pinned loads were found
    assert all("operand regs  22" in l for l in lines), r.stdout
    assert r.returncode == 0, r.stdout + r.stderr

"""The LDS-DMA weight-gradient kernels hold their accumulators and fragments in registers: wg_rect_mfma
(csrc/wgrad_kernels.h) is plain `inline`, and a build that left it as a call would pass its array arguments
through scratch.  The gfx950 listing must show ScratchSize 0 for every k_wgrad_dma / k_wgrad_tr / k_wgrad_mix
instantiation (hipcc cross-compiles, no GPU needed)."""
import os
import shutil
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))


@pytest.mark.skipif(shutil.which("/opt/rocm/bin/hipcc") is None, reason="hipcc not installed")
def test_wgrad_dma_kernels_use_no_scratch(tmp_path):
    import kernel_isa_diff

    csrc = os.path.join(REPO, "marl-maze_amd", "csrc")
    out = str(tmp_path / "k.s")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                    "--cuda-device-only", "-S", "-I", os.path.join(REPO, "include"), "-I", csrc, "-o", out,
                    os.path.join(csrc, "x3mlp.hip")], check=True, stderr=subprocess.DEVNULL, timeout=600)
    ks = {n: info for n, (_, info) in kernel_isa_diff.kernels(out).items()
          if any(k in n for k in ("11k_wgrad_dma", "10k_wgrad_tr", "11k_wgrad_mix"))}
    assert len(ks) == 4, sorted(ks)  # dma <17, 9> and <17, 8>, tr <17, 9>, mix <17, 8>
    for name, info in ks.items():
        assert info["ScratchSize"] == 0, (name, info)

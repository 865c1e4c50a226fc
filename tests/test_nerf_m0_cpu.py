"""The split NeRF kernels that set M0 for their LDS-DMA without handing it back (csrc/nerf_split_chain.h, owns_m0) may do so only while the
compiler emits no instruction of its own that reads or writes M0 in them: M0 is a reserved register, a clobber of it is not honoured.
`scripts/kstep_gaps.py --m0` checks that on the device assembly -- every instruction that names M0 and every LDS-DMA stands in an
inline-asm block of the project, and M0 is only written there, never read or saved.  This test compiles the two kernel files with the
product's flags (`-S`, device only; no GPU) and runs the mode on every kernel that dropped the save / restore, and on the two that kept
the compiler's LDS-DMA, which the mode must tell apart."""
import os
import shutil
import subprocess
import sys
from pathlib import Path

import pytest

from nerfmatch_amd import build as nm_build

ROOT = Path(__file__).resolve().parents[1]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
OWNERS = {"nerf_fwd_bf16": ("nerf_fwd_bf16x3_kernel", "nerf_fwd_fp16x3_kernel", "nerf_fwd_fp16x3_tap7_kernel"),
          "nerf_points_bf16": ("nerf_points_fwd_kernel", "nerf_points_fwd_rays_kernel")}
KEEPERS = {"nerf_fwd_bf16": ("nerf_fwd_fp16x1_kernel",), "nerf_points_bf16": ("nerf_points_bwd_kernel",)}

pytestmark = pytest.mark.skipif(not (Path(HIPCC).exists() or shutil.which(HIPCC)), reason="no hipcc")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = tmp_path_factory.mktemp("m0")
    flags = [f for f in nm_build.FLAGS if f != "-fPIC"]
    procs = {}
    for stem in OWNERS:
        cmd = [HIPCC, *flags, "-S", "--cuda-device-only", f"-I{nm_build.CSRC}", f"-I{ROOT / 'include'}", str(nm_build.CSRC / f"{stem}.hip"),
               "-o", str(out / f"{stem}.s")]
        procs[stem] = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    for stem, p in procs.items():
        log, _ = p.communicate()
        assert p.returncode == 0, log[-2000:]
    return out


def _m0(asm, stem, kernel):
    return subprocess.run([sys.executable, str(ROOT / "scripts" / "kstep_gaps.py"), str(asm / f"{stem}.s"), kernel, "--m0"], capture_output=True, text=True)


@pytest.mark.parametrize("stem,kernel", [(s, k) for s, ks in OWNERS.items() for k in ks])
def test_kernel_owns_m0(asm, stem, kernel):
    res = _m0(asm, stem, kernel)
    print(res.stdout)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "global_load_lds" in res.stdout and " 0 not of the project's own pattern" in res.stdout


@pytest.mark.parametrize("stem,kernel", [(s, k) for s, ks in KEEPERS.items() for k in ks])
def test_a_kernel_with_the_compilers_lds_dma_is_told_apart(asm, stem, kernel):
    res = _m0(asm, stem, kernel)
    assert res.returncode == 1, res.stdout + res.stderr
    assert "COMPILER" in res.stdout and "s_mov_b32 sN, m0" in res.stdout  # its asm pieces save M0 and hand it back

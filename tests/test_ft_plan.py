"""Tile plan of the feature-GEMM statistics kernel (no GPU): tests/cpp/ft_plan_test.cpp includes the plan helpers of
lc_kernels.h, is compiled for the host with hipcc and checks every instance launch_ss_feat can take."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def test_feature_gemm_tile_plan(tmp_path):
    from libcluster_amd import build as b

    exe = tmp_path / "ft_plan_test"
    cmd = [b._hipcc(), "-std=c++17", "-O1", f"-I{ROOT / 'libcluster_amd' / 'csrc'}", str(ROOT / "tests/cpp/ft_plan_test.cpp"),
           "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "ok " in r.stdout
    # the headline instance: 135 tiles (141 with the patch deal), no SIMD above 17
    assert "DP  64 DC  64 NQ  8: 135 tiles,  2 blocks of 8 waves, <= 9 per wave, busiest SIMD 17" in r.stdout

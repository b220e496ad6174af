"""The check's kernel file as a file: check_kernels.hip compiles for gfx950 as a
translation unit of its own, and k_check_values -- the piece loop without a
destination -- keeps its registers: no scratch, nothing spilled, and the
occupancy this compile gives (40 VGPRs, 8 waves per SIMD; a
regression pin, not a target).  The other three kernels of the file are held
to no scratch and no spills."""
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_kernel_files_cpu import CSRC, FLAGS, hipcc  # noqa: E402

OCCUPANCY = {"k_check_valuesE": 8}
KERNELS = ("k_check_lengthsE", "k_check_valuesE", "k_check_approxE", "k_check_reportE")


def test_check_kernels_registers_and_scratch(tmp_path):
    assert os.path.exists(os.path.join(CSRC, "check_kernels.hip")) and os.path.exists(os.path.join(CSRC, "check_plan.hpp"))
    src = tmp_path / "forms.hip"
    src.write_text('#include "check_kernels.hip"\n')
    r = subprocess.run([hipcc(), *FLAGS, "-c", "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "forms.o"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    seen, name = {}, None
    for line in r.stderr.splitlines():
        if "remark:" not in line:
            continue
        key, _, val = line.split("remark:", 1)[1].rsplit("[-Rpass", 1)[0].strip().partition(":")
        if key == "Function Name":
            name = val.strip()
            seen[name] = {}
        elif name is not None:
            seen[name][key.strip()] = val.strip()
    for kernel in KERNELS:
        mine = [u for n, u in seen.items() if kernel in n]
        assert len(mine) == 1, (kernel, sorted(seen))
        u = mine[0]
        print(kernel, "VGPRs", u["VGPRs"], "waves/SIMD", u["Occupancy [waves/SIMD]"])
        assert int(u["ScratchSize [bytes/lane]"]) == 0 and int(u["VGPRs Spill"]) == 0 and int(u["SGPRs Spill"]) == 0, (kernel, u)
        if kernel in OCCUPANCY:
            assert int(u["Occupancy [waves/SIMD]"]) == OCCUPANCY[kernel], (kernel, u)

"""The registers of the dump kernels (bsdb_amd/csrc/dump_kernels.hip) as the
compiler reports them for gfx950: k_db_records and k_dump_text keep no
scratch and spill nothing.  Their VGPRs and waves per SIMD are printed beside
k_text_pack<true>'s from the same compile (DESIGN §3.9 records them).  That
the file compiles as a unit of its own is tests/test_kernel_files_cpu.py's."""
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_kernel_files_cpu import FLAGS, hipcc

KERNELS = ("k_db_recordsE", "k_dump_textE")
BESIDE = "k_text_packILb1E"


def test_dump_kernels_registers_and_scratch(tmp_path):
    src = tmp_path / "forms.hip"
    src.write_text('#include "dump_kernels.hip"\n#include "text_kernels.hip"\nnamespace bsdb {\n'
                   "template __global__ void k_text_pack<true>(TextPack);\n}\n")
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
    for kernel in KERNELS + (BESIDE,):
        mine = [u for n, u in seen.items() if kernel in n]
        assert len(mine) == 1, (kernel, sorted(seen))
        u = mine[0]
        print(kernel, "VGPRs", u["VGPRs"], "waves/SIMD", u["Occupancy [waves/SIMD]"])
        if kernel in KERNELS:
            assert int(u["ScratchSize [bytes/lane]"]) == 0 and int(u["VGPRs Spill"]) == 0 and int(u["SGPRs Spill"]) == 0, (kernel, u)

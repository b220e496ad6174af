"""The registers of the merge kernels (bsdb_amd/csrc/merge_kernels.hip) as the
compiler reports them for gfx950, from one compile: none of them keeps scratch
or spills.  Their VGPRs and waves per SIMD are printed beside
k_text_pack<true>'s and k_text_pack_blocked's from the same compile (DESIGN
§3.11 records them); the text pack, which this work must leave as it was, keeps
its 58 VGPRs, 8 waves per SIMD and no scratch.  That the file compiles as a
unit of its own is shown here too."""
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_kernel_files_cpu import FLAGS, hipcc

KERNELS = ("k_merge_statusE", "k_rec_sizesE", "k_rec_packILb1E", "k_rec_packILb0E", "k_rec_pack_blockedE", "k_rec_outputsE")
BESIDE = ("k_text_packILb1E", "k_text_pack_blockedE")
TEXT_PACK = {"VGPRs": 58, "Occupancy [waves/SIMD]": 8, "ScratchSize [bytes/lane]": 0}


def test_merge_kernels_registers_and_scratch(tmp_path):
    src = tmp_path / "forms.hip"
    src.write_text('#include "merge_kernels.hip"\nnamespace bsdb {\n'
                   "template __global__ void k_rec_pack<true>(RecPack);\ntemplate __global__ void k_rec_pack<false>(RecPack);\n"
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
    for kernel in KERNELS + BESIDE:
        mine = [u for n, u in seen.items() if kernel in n]
        assert len(mine) == 1, (kernel, sorted(seen))
        u = mine[0]
        print(kernel, "VGPRs", u["VGPRs"], "waves/SIMD", u["Occupancy [waves/SIMD]"], "scratch", u["ScratchSize [bytes/lane]"])
        if kernel in KERNELS:
            assert int(u["ScratchSize [bytes/lane]"]) == 0 and int(u["VGPRs Spill"]) == 0 and int(u["SGPRs Spill"]) == 0, (kernel, u)
        if kernel == BESIDE[0]:
            assert {k: int(u[k]) for k in TEXT_PACK} == TEXT_PACK, u

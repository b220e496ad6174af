"""The kernel sources as files: every kernel file and header under
bsdb_amd/csrc compiles for gfx950 as a translation unit of its own (it
includes what it uses; the library builds them in one unit, where the order of
the includes would hide a missing one), and the four kernels of the piece loop
(piece_copy.hpp) keep their registers: no scratch, nothing spilled, and the
occupancy they had as three hand-kept copies of the loop."""
import glob
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bsdb_amd", "csrc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fgpu-flush-denormals-to-zero", "-Wall", "-Werror",
         "-Wno-unused-function", "--cuda-device-only", "-I", CSRC]
FILES = sorted(os.path.basename(p) for pat in ("*_kernels.hip", "*.hpp") for p in glob.glob(os.path.join(CSRC, pat)))

# waves per SIMD before the piece loop had one home (VGPRs then: 48, 55, 48, 76)
# (keyed by a piece of the mangled name)
OCCUPANCY = {"k_get_gatherE": 8, "k_text_packILb1E": 8, "k_text_packILb0E": 8, "k_text_pack_blockedE": 6}


def hipcc():
    cc = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")) if c and os.path.exists(c)),
              None)
    if cc is None:
        pytest.skip("no hipcc on this machine")
    return cc


def test_every_file_is_listed():
    assert len(FILES) >= 18 and {"piece_copy.hpp", "piece_plan.hpp", "get_kernels.hip", "gov_kernels.hip"} <= set(FILES)


@pytest.mark.parametrize("name", FILES)
def test_file_compiles_on_its_own(tmp_path, name):
    src = tmp_path / "unit.hip"
    src.write_text(f'#include "{name}"\n')
    # (the hipcc wrapper passes --hip-link, which a run that links nothing does not use)
    r = subprocess.run([hipcc(), *FLAGS, "-Wno-unused-command-line-argument", "-fsyntax-only", str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_piece_kernels_registers_and_scratch(tmp_path):
    src = tmp_path / "forms.hip"
    src.write_text('#include "get_kernels.hip"\n#include "text_blocked_kernels.hip"\nnamespace bsdb {\n'
                   "template __global__ void k_text_pack<true>(TextPack);\n"
                   "template __global__ void k_text_pack<false>(TextPack);\n}\n")
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
    for kernel, floor in OCCUPANCY.items():
        mine = [u for n, u in seen.items() if kernel in n]
        assert len(mine) == 1, (kernel, sorted(seen))
        u = mine[0]
        print(kernel, "VGPRs", u["VGPRs"], "waves/SIMD", u["Occupancy [waves/SIMD]"])
        assert int(u["ScratchSize [bytes/lane]"]) == 0 and int(u["VGPRs Spill"]) == 0 and int(u["SGPRs Spill"]) == 0, (kernel, u)
        assert int(u["Occupancy [waves/SIMD]"]) >= floor, (kernel, u)

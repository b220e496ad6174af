"""The piece-copy kernels (piece_copy.hpp: k_get_gather, k_text_pack,
k_text_pack_blocked) and the text split and block placement kernels, run on
the host under ASan + UBSan without a GPU.

tests/piece_host_check.cpp includes the kernel files unchanged; the header
tests/hostwave/hip/hip_runtime.h stands in for HIP's and runs a workgroup as
fibers.  The program is built with the ROCm clang++ (the kernel files need
clang's extensions), the sanitizer runtimes linked into it, and started as a
program of its own, as tests/test_get_plan_cpu.py does for the plan headers.
It gives every input an allocation of exactly its length and every output a
view between guard bytes, so a read or a write one byte outside what a kernel
was told is a report here -- where on a GPU it is slack of a larger allocation
and says nothing.

Ground truth is Python's: slices of the image formula for the gather,
tests/text_rule.py for the compact pack and the split, kvfiles.write_blocked
per run for the blocked pack (as tests/test_text_blocked_gpu.py's
oracle_chunk).  Valid cases are compared byte for byte.  Hostile cases
(offsets that are no scan, sources past the image, descriptors with lengths no
record has and positions past the text) must leave no report and no dead guard
byte, and still give what the comments of the kernels promise: see
piece_cases.gather_promised and piece_cases.described_records.

test_mutation shows that this harness notices a subtly wrong kernel: nine
one-line edits of the library's sources, each built against a copy and each
required to fail at least one case.

What the emulation does not prove is listed in the shim's opening comment: the
memory model, races of lanes through LDS or global memory, code generation,
speed.  The GPU suite stays the judge of the real kernels."""
import concurrent.futures
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import piece_cases as P  # noqa: E402
import text_rule as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "piece_host_check.cpp")
SHIM = os.path.join(ROOT, "tests", "hostwave")
CSRC = os.path.join(ROOT, "bsdb_amd", "csrc")
FLAGS = ["-x", "c++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread"]
GUARD = 0xA5


def find_compiler():
    """The ROCm clang++: next to HIPCC (or under its llvm/bin), the usual place, or the path's."""
    cands = []
    for hipcc in (os.environ.get("HIPCC"), shutil.which("hipcc")):
        if hipcc:
            d = os.path.dirname(os.path.realpath(hipcc))
            cands += [os.path.join(d, "clang++"), os.path.join(d, "..", "llvm", "bin", "clang++"),
                      os.path.join(d, "..", "lib", "llvm", "bin", "clang++")]
    if os.environ.get("ROCM_PATH"):
        cands.append(os.path.join(os.environ["ROCM_PATH"], "llvm", "bin", "clang++"))
    cands += ["/opt/rocm/llvm/bin/clang++", shutil.which("clang++")]
    return next((c for c in cands if c and os.path.isfile(c) and os.access(c, os.X_OK)), None)


def build(cxx, exe, csrc=CSRC):
    return subprocess.run([cxx] + FLAGS + ["-I", SHIM, "-I", csrc, "-o", exe, SRC], capture_output=True, text=True)


def encode(case):
    def tok(v):
        if isinstance(v, (bytes, bytearray)):
            return bytes(v).hex()
        if isinstance(v, (list, tuple)):
            return ",".join(str(int(x)) for x in v)
        return str(v)
    return " ".join(f"{k}={tok(v)}" for k, v in case.items() if not k.startswith("_"))


def run(exe, cases):
    """(exit status, one dict per case that ran, the end of stderr)."""
    r = subprocess.run([exe], input="".join(encode(c) + "\n" for c in cases), capture_output=True, text=True, timeout=300)
    return r.returncode, [json.loads(line) for line in r.stdout.splitlines() if line.endswith("}")], r.stderr[-3000:]


@pytest.fixture(scope="module")
def cxx():
    c = find_compiler()
    if c is None:
        pytest.skip("no clang++ on this machine (the kernel files need clang's extensions)")
    return c


@pytest.fixture(scope="module")
def exe(cxx, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("piece_host") / "piece_host_check")
    r = build(cxx, path)
    assert r.returncode == 0, r.stderr[-3000:]
    rc, _, err = run(path, [])
    if rc != 0:
        pytest.skip("the sanitized program does not start in this environment: " + err.strip()[-300:])
    return path


def run_ok(exe, cases):
    rc, out, err = run(exe, cases)
    assert rc == 0, err                       # no sanitizer report
    assert len(out) == len(cases)
    return out


# ---- the checks: each raises AssertionError on the first case that is wrong ----------------------------------

def check_gather_valid(cases, outs):
    for c, o in zip(cases, outs):
        want = b"".join(P.image_bytes_at(s * c["scale"], l, c["image_bytes"]) for s, l in zip(c["src"], c["_vlens"]))
        assert len(want) == c["value_bytes"]
        assert o["guard"] == 1, ("guard", c["mis"], c["_vlens"])
        assert bytes.fromhex(o["out"]) == want, (c["mis"], c["scale"], c["_vlens"])


def check_gather_hostile(cases, outs):
    covered = 0
    for c, o in zip(cases, outs):
        got = bytes.fromhex(o["out"])
        assert o["guard"] == 1 and len(got) == c["value_bytes"], ("guard", c["_family"])
        for at, byte in P.gather_promised(c):
            assert got[at] == byte, (c["_family"], at, c["voff"], c["src"])
            covered += 1
    return covered


def check_pack(cases, outs, tmp):
    """Valid and hostile alike: the records are those the descriptors describe after the cut."""
    import test_text_blocked_gpu as G
    for c, o in zip(cases, outs):
        name = (c["mode"], c["_name"], c["mis"])
        assert "refused" not in o, name + (o,)      # sizes past what the largest records need
        recs = P.described_records(c)
        parts, B, before = c["parts"], c.get("B", 0), c["before"]
        bound = R.run_bounds(len(recs), parts)
        rrecs = [(0, k, 0, v) for k, v in recs]
        if B:
            image, runs, addr = G.oracle_chunk(tmp, recs, parts, B, before)
            addr = [int(a) for a in addr]
        else:
            image, offs = R.image_of(rrecs)
            offs.append(len(image))
            runs = [offs[bound[p + 1]] - offs[bound[p]] for p in range(parts)]
            addr = [p << 56 | (before[p] + offs[r] - offs[bound[p]]) for p in range(parts) for r in range(bound[p], bound[p + 1])]
        # the sizes are the cut lengths': 3 + min(klen, 255) + min(vlen, 32 510) a record
        sizes = [3 + min(kl, 255) + min(vl, 32510) for kl, vl in zip(c["klen"], c["vlen"])]
        assert [3 + len(k) + len(v) for k, v in recs] == sizes
        if not B:
            assert len(image) == sum(sizes)
        assert o["guard"] == 1, ("guard",) + name
        assert o["run_bytes"] == runs, name
        got = bytes.fromhex(o["image"])
        assert len(got) == len(image), name
        if got != image:
            bad = next(i for i in range(len(image)) if got[i] != image[i])
            raise AssertionError(name + ("image byte", bad, got[bad], image[bad]))
        assert o["addr"] == addr, name
        assert bytes.fromhex(o["blob"]) == b"".join(k for k, _ in recs), name
        assert o["off"] == [0] + np.cumsum([len(k) for k, _ in recs]).tolist(), name
        v8, vl = R.value_heads(rrecs)
        assert o["value8"] == [int(x) for x in v8] and o["value_len"] == [int(x) for x in vl], name


def check_split(cases, outs):
    for c, o in zip(cases, outs):
        recs, want = R.restate(c["text"], bytes([c["sep"]]))
        rep = dict(zip(R.FIELDS + ("chunks",), o["report"]))
        assert o["guard"] == 1, ("guard", c["_name"])
        assert {k: rep[k] for k in R.FIELDS} == want, (c["_name"], rep, want)
        assert rep["chunks"] == (1 if c["text"] else 0)
        exp = [[kp, len(k), vp, len(v)] for kp, k, vp, v in recs]
        assert [list(x) for x in zip(o["kpos"], o["klen"], o["vpos"], o["vlen"])] == exp, c["_name"]


# ---- the cases on the library as it is -------------------------------------------------------------------------

def test_gather_valid(exe):
    cases = P.gather_valid()
    assert len(P.gather_enumeration()) == 16 * (7 + 49 + 343 - 3)
    check_gather_valid(cases, run_ok(exe, cases))


def test_gather_offsets_that_are_no_scan(exe):
    cases = P.gather_hostile()
    assert {c["_family"] for c in cases} == {"random", "below_total", "every_second", "decreasing", "tail_zeros", "tail_ones",
                                             "src"}
    assert {c["scale"] for c in cases} == {1, 8} and all(1 <= c["image_bytes"] <= 300 for c in cases)
    covered = check_gather_hostile(cases, run_ok(exe, cases))
    assert covered > 1000                     # the promise is not empty: tail_ones and src predict whole values


def test_pack(exe, tmp_path):
    cases = P.pack_valid()
    check_pack(cases, run_ok(exe, cases), str(tmp_path))
    image = bytes.fromhex(run_ok(exe, [c for c in cases if c["_name"] == "value256_alone"])[0]["image"])
    assert image[:3] == bytes([3, 1, 0])      # the 256-byte value's header: its second byte is not 0


def test_pack_blocked(exe, tmp_path):
    cases = P.pack_valid(B=P.PAGE) + P.blocked_table()
    check_pack(cases, run_ok(exe, cases), str(tmp_path))


@pytest.mark.parametrize("B", [0, P.PAGE], ids=["compact", "blocked"])
def test_pack_hostile_descriptors(exe, tmp_path, B):
    cases = P.pack_hostile(B=B)
    text = cases[0]["text"]
    # what the families must hold: lengths no record has, positions at and past the text's end
    assert {256, 32511, 65536, P.U32 - 1} <= {x for c in cases for x in c["klen"]} & {x for c in cases for x in c["vlen"]}
    assert {len(text) - 1, len(text), len(text) + 1, P.U32 - 1} <= ({x for c in cases for x in c["kpos"]} &
                                                                     {x for c in cases for x in c["vpos"]})
    check_pack(cases, run_ok(exe, cases), str(tmp_path))


def test_split(exe):
    cases = P.split_cases()
    assert sum(len(c["text"]) % 16 != 0 for c in cases) > 10
    check_split(cases, run_ok(exe, cases))


def test_the_shim_itself(cxx, exe, tmp_path):
    """A shuffle that one lane of a wave skips, so that it waits at the workgroup's barrier while its wave waits
    for it, aborts with a message; lanes that have returned do not hold a barrier up, a ballot sees 0 from them
    and a shuffle from one returns the caller's own value."""
    src = tmp_path / "shim_check.cpp"
    src.write_text(r'''
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
__global__ void k_skip(int) { if (threadIdx.x != 5) __shfl(1, 0, 64); __syncthreads(); }
__global__ void k_ok(unsigned long long *out) {
    __shared__ unsigned sum[4];
    if (threadIdx.x >= 70 && threadIdx.x < 128) return;          // lanes 6 .. 63 of wave 1 leave
    const unsigned long long b = __ballot(threadIdx.x % 3 == 0);
    const unsigned from = __shfl(threadIdx.x, 9, 64);              // lane 9 of wave 1 has left
    const unsigned up = __shfl_up(threadIdx.x, 1, 64), x = __shfl_xor(threadIdx.x, 1, 64);
    if ((threadIdx.x & 63) == 0) sum[threadIdx.x >> 6] = 0;
    __syncthreads();
    atomicAdd(&sum[threadIdx.x >> 6], 1u);
    __syncthreads();
    out[4 * threadIdx.x] = b, out[4 * threadIdx.x + 1] = from, out[4 * threadIdx.x + 2] = (unsigned long long)up << 32 | x;
    out[4 * threadIdx.x + 3] = sum[threadIdx.x >> 6] | (unsigned long long)blockIdx.x << 32 | (unsigned long long)gridDim.x << 48;
}
int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "skip")) hostwave::launch(1, 256, k_skip, 0);
    static unsigned long long out[4 * 256];
    for (int rep = 0; rep < 2; ++rep) hostwave::launch(3, 256, k_ok, out);   // (the fibers are used again)
    for (int t = 0; t < 256; ++t) printf("%llu %llu %llu %llu\n", out[4 * t], out[4 * t + 1], out[4 * t + 2], out[4 * t + 3]);
    return 0;
}
''')
    exe = str(tmp_path / "shim_check")
    r = subprocess.run([cxx] + FLAGS + ["-I", SHIM, "-o", exe, str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    ok = subprocess.run([exe], capture_output=True, text=True)
    assert ok.returncode == 0, ok.stderr[-3000:]
    rows = [[int(x) for x in line.split()] for line in ok.stdout.splitlines()]
    assert len(rows) == 256
    for t, (b, frm, upx, s) in enumerate(rows):
        lane, wave = t & 63, t >> 6
        if 70 <= t < 128:
            assert (b, frm, upx, s) == (0, 0, 0, 0)
            continue
        live = range(6) if wave == 1 else range(64)
        assert b == sum(1 << l for l in live if (64 * wave + l) % 3 == 0), t
        assert frm == (t if wave == 1 else 64 * wave + 9), t
        assert upx >> 32 == (t - 1 if lane else t) and upx & 0xFFFFFFFF == t ^ 1, t
        assert s == (6 if wave == 1 else 64) | 2 << 32 | 3 << 48, t       # the last workgroup's: blockIdx 2 of 3
    bad = subprocess.run([exe, "skip"], capture_output=True, text=True)
    assert bad.returncode != 0 and "a barrier that cannot complete" in bad.stderr, bad.stderr[-500:]


# ---- mutations: the harness notices a subtly wrong kernel -----------------------------------------------------

def _gather_some():
    return [c for c in P.gather_enumeration() if c["mis"] in (0, 5)] + P.gather_empty_runs()


def _named(prefix):
    return lambda: [c for c in P.pack_valid() if c["_name"].startswith(prefix)]


CASES = {
    "gather_valid": (_gather_some, check_gather_valid),
    "gather_hostile": (P.gather_hostile, check_gather_hostile),
    "value_ends_the_text": (_named("value_ends_the_text"), None),
    "value256": (_named("value256"), None),
    "pack_hostile": (P.pack_hostile, None),
    "split_no_multiple_of_16": (lambda: [c for c in P.split_cases() if len(c["text"]) % 16], check_split),
}

MUTATIONS = [
    # (id, file, what is there, what replaces it, the cases that must notice, how: "any" = wrong bytes, a dead guard or
    # a sanitizer report; "guard" = a dead guard byte; "asan" = an AddressSanitizer report)
    ("owner_search_strict", "piece_copy.hpp", "if (off[mid] <= o) lo = mid;", "if (off[mid] < o) lo = mid;", "gather_valid", "any"),
    ("put_drops_the_high_half", "piece_copy.hpp", "            if (j) hi |= x >> (64 - 8 * j);\n", "", "gather_valid", "any"),
    ("end_of_not_cut", "piece_copy.hpp", "return e < out_bytes ? e : out_bytes;", "return e;", "gather_valid", "guard"),
    ("runs_no_break", "piece_copy.hpp", "        if (rs > o || re <= o) break;", "        ;", "gather_hostile", "any"),
    ("piece_count_ignores_misalignment", "piece_plan.hpp", "(misalign & 15)", "0", "gather_valid", "any"),
    ("bounded_reader_reads_a_whole_dword", "spooky_dev.hpp", "if (x + 4 <= limit)", "if (x < limit)", "value_ends_the_text",
     "asan"),
    ("classify_reads_a_whole_piece", "text_kernels.hip", "if (p0 + 16 <= bytes)", "if (p0 < bytes)", "split_no_multiple_of_16",
     "asan"),
    ("header_bytes_swapped", "text_kernels.hip", "(uint64_t)(vl >> 8) << 8 | (uint64_t)(vl & 0xFF) << 16",
     "(uint64_t)(vl & 0xFF) << 8 | (uint64_t)(vl >> 8) << 16", "value256", "any"),
    ("key_length_uncut", "text_kernels.hip", "return klen < TEXT_MAX_KEY ? klen : TEXT_MAX_KEY;", "return klen;", "pack_hostile",
     "any"),
]


@pytest.fixture(scope="module")
def mutants(cxx, exe, tmp_path_factory):
    """Every mutation's program, built against a copy of the sources with the one substitution; built together."""
    top = tmp_path_factory.mktemp("mutants")

    def make(m):
        name, fname, old, new = m[:4]
        d = str(top / name)
        shutil.copytree(CSRC, d, ignore=shutil.ignore_patterns("*.o", "*.so", "*.so.*", "*.a"))
        path = os.path.join(d, fname)
        text = open(path).read()
        if text.count(old) != 1:              # a refactor moved the line: the entry must follow it
            return name, None, f"{fname}: {old!r} occurs {text.count(old)} times, not once"
        with open(path, "w") as f:
            f.write(text.replace(old, new))
        r = build(cxx, os.path.join(d, "piece_host_check"), d)
        return name, os.path.join(d, "piece_host_check"), r.stderr[-3000:] if r.returncode else None

    with concurrent.futures.ThreadPoolExecutor(max(1, min(4, os.cpu_count() or 1))) as pool:
        return {name: (path, err) for name, path, err in pool.map(make, MUTATIONS)}


@pytest.mark.parametrize("name", [m[0] for m in MUTATIONS])
def test_mutation(mutants, tmp_path, name):
    """The one substitution makes at least one of the named cases fail, in the named way."""
    path, err = mutants[name]
    assert err is None, err
    which, how = next(m[4:] for m in MUTATIONS if m[0] == name)
    make, check = CASES[which]
    cases = make()
    assert cases
    rc, outs, stderr = run(path, cases)
    if how == "asan":
        assert rc != 0 and "AddressSanitizer" in stderr, (rc, stderr)
    elif how == "guard":
        assert rc == 0 and any(o["guard"] == 0 for o in outs), (rc, stderr)
    elif rc != 0:
        assert "Sanitizer" in stderr or "runtime error" in stderr, stderr   # a report, not a program that does not start
    else:
        assert len(outs) == len(cases)
        with pytest.raises(AssertionError):
            check(cases, outs) if check else check_pack(cases, outs, str(tmp_path))

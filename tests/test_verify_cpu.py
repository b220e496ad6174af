"""The database check's C ABI, bindings and JNI seam without a device: what the
header declares, argument errors before any device call, the report's field
order, and the Java native with its shim."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "bsdb_amd", "libbsdb_mi355x.so")
HDR = os.path.join(ROOT, "include", "bsdb_mi355x.h")
FUNCS = ["bsdb_dev_verify_fixed", "bsdb_dev_verify_var", "bsdb_mph_verify_index_fixed", "bsdb_mph_verify_index_var",
         "bsdb_kv_verify_index"]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)


def test_header_declares_the_five_functions_and_the_report_size():
    h = _header()
    for f in FUNCS:
        assert re.search(r"\bint\s+" + f + r"\s*\(", h), f
    assert re.search(r"#define\s+BSDB_VERIFY_WORDS\s+8\b", h)
    assert re.search(r"#define\s+BSDB_ABI_VERSION\s+6\b", h)  # additive: the ABI number stays


def test_null_arguments_are_einval_without_a_device():
    """NULL out / context / MPHF: -22 before any device call (this runs where no GPU is)."""
    import bsdb_amd.native as N
    L = N.lib()
    out = (C.c_uint64 * 8)()
    p = b"/nonexistent/index.db"
    # NULL context, then NULL out with a NULL context
    assert L.bsdb_dev_verify_fixed(None, None, 13, 0, None, 0, 0, 0, None, None, 0, 1, None, None, 0, None, 0, 0, None,
                                   None, C.addressof(out), None) == -22
    assert L.bsdb_dev_verify_fixed(None, None, 13, 0, None, 0, 0, 0, None, None, 0, 1, None, None, 0, None, 0, 0, None,
                                   None, None, None) == -22
    assert L.bsdb_dev_verify_var(None, None, 0, None, 0, None, 0, 0, 0, None, None, 0, 1, None, None, 0, None, 0, 0,
                                 None, None, None, None) == -22
    # NULL MPHF, with and without out
    for o in (C.addressof(out), None):
        assert L.bsdb_mph_verify_index_fixed(None, None, 13, 0, None, None, None, 0, p, None, 0, o) == -22
        assert L.bsdb_mph_verify_index_var(None, None, None, 0, None, None, None, 0, p, None, 0, o) == -22
        assert L.bsdb_kv_verify_index(None, b"/nonexistent/kv.db", 1, 0, 4096, 1, 0, p, None, 0, o) == -22
    assert list(out) == [0] * 8  # nothing was written


def test_report_fields_follow_the_header_word_order():
    """The dict's fields are the header's words [0..7], in order."""
    import bsdb_amd.native as N
    txt = open(HDR).read()
    doc = txt[txt.index("The report is uint64_t out[BSDB_VERIFY_WORDS]"):]
    doc = doc[: doc.index("bsdb_dev_verify_*:")]
    words = {int(m.group(1)): m.group(2) for m in re.finditer(r"\[(\d)\]\s+([a-z_]+(?: [a-z]+)?)", doc)}
    want = {0: "records seen", 1: "rejected", 2: "in_window", 3: "wrong_addr", 4: "wrong_value", 5: "min_bad_addr",
            6: "structure flags", 7: "windows used"}
    assert words == want
    assert N.VERIFY_WORDS == 8 and len(N.VERIFY_FIELDS) == 8
    for i, name in enumerate(N.VERIFY_FIELDS):
        assert want[i].replace(" ", "_").startswith(name) or name in want[i].split(), (i, name)
    out = (C.c_uint64 * 8)(*range(10, 18))
    rep = N._verify_report("f", N.BSDB_EVERIFY, out)
    assert [rep[k] for k in N.VERIFY_FIELDS] == list(range(10, 18)) and rep["ok"] is False
    assert list(rep)[:8] == list(N.VERIFY_FIELDS)
    assert N._verify_report("f", 0, out)["ok"] is True
    with pytest.raises(N.BsdbError):
        N._verify_report("f", -9, out)


def test_java_native_and_shim():
    java = open(os.path.join(ROOT, "jni", "GpuBuild.java")).read()
    assert re.search(r"public\s+static\s+native\s+boolean\s+kvVerifyIndex\s*\([^)]*long\[\]\s+report\s*\)", java, re.S)
    shim = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "jni", "gpu_jni.c")).read(), flags=re.S)
    body = shim[shim.index("JF(kvVerifyIndex)"):]
    assert "bsdb_kv_verify_index(" in body
    assert "utf(env, kv)" in body and "unutf(env, kv, k)" in body  # the null-safe string helpers
    assert "BSDB_EVERIFY" in body and "CHECK(rc)" in body          # EVERIFY is an answer, the rest throws
    writer = open(os.path.join(ROOT, "jni", "GpuBSDBWriter.java")).read()
    assert re.search(r"public\s+long\[\]\s+verify\s*\(\s*\)", writer) and "GpuBuild.kvVerifyIndex(" in writer

"""The duplicate finder's C ABI, bindings and JNI seam without a device: what
the header declares, the exports, the ctypes signatures, argument errors
before any device call, the Java native with its shim, and the exception a
failed build raises."""
import ctypes as C
import fnmatch
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "bsdb_mi355x.h")
FUNCS = ["bsdb_dev_find_duplicates_fixed", "bsdb_dev_find_duplicates_var", "bsdb_dev_find_duplicates_sig",
         "bsdb_dev_classify_pairs_fixed", "bsdb_dev_classify_pairs_var", "bsdb_find_duplicates_fixed",
         "bsdb_find_duplicates_var", "bsdb_builder_find_duplicates", "bsdb_kv_find_duplicates"]
CONSTS = {"BSDB_DUP_WORDS": 4, "BSDB_DUP_SAME_KEY": 0, "BSDB_DUP_COLLISION": 1, "BSDB_DUP_UNCOMPARED": 2,
          "BSDB_DUP_LIST_FULL": 1, "BSDB_DUP_PARTIAL": 2}


def _strip(s):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", s, flags=re.S))


def _split_args(s):
    out, depth, cur = [], 0, ""
    for ch in s:
        depth += {"(": 1, "[": 1, ")": -1, "]": -1}.get(ch, 0)
        if ch == "," and depth == 0:
            out.append(cur.strip())
            cur = ""
        else:
            cur += ch
    return out + ([cur.strip()] if cur.strip() else [])


def _header_args(name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;{]*?)\)\s*;", _strip(open(HDR).read()), re.S)
    assert m, name
    return _split_args(m.group(1))


def test_header_declares_the_functions_and_constants():
    h = _strip(open(HDR).read())
    for f in FUNCS:
        assert re.search(r"\bint\s+" + f + r"\s*\(", h), f
    for name, value in CONSTS.items():
        assert re.search(r"#define\s+" + name + r"\s+" + str(value) + r"\b", h), name
    assert re.search(r"#define\s+BSDB_ABI_VERSION\s+6\b", h)  # additive: the ABI number stays
    assert re.search(r"#define\s+BSDB_EDUP\s+\(-17\)", h)


def test_every_name_is_exported_and_bound():
    import bsdb_amd.native as N
    patterns = re.findall(r"global:\s*([^;]+);", open(os.path.join(ROOT, "bsdb_amd", "csrc", "exports.map")).read())
    L = N.lib()
    sigs = {name: (res, args) for name, res, args in N.SIGNATURES}
    for f in FUNCS:
        assert any(fnmatch.fnmatch(f, p.strip()) for p in patterns), f
        assert hasattr(L, f), f
        assert f in sigs and sigs[f][0] is C.c_int, f
        assert len(sigs[f][1]) == len(_header_args(f)), f  # the header's arity
    assert (N.DUP_WORDS, N.DUP_LIST_FULL, N.DUP_PARTIAL) == (4, 1, 2)
    assert (N.DUP_SAME_KEY, N.DUP_COLLISION, N.DUP_UNCOMPARED) == (0, 1, 2)
    assert N.DUP_FIELDS == ("found", "collisions", "flags", "keys")


def test_null_arguments_are_einval_without_a_device():
    import bsdb_amd.native as N
    L = N.lib()
    rep = (C.c_uint64 * 4)(9, 9, 9, 9)
    r = C.addressof(rep)
    assert L.bsdb_dev_find_duplicates_fixed(None, None, 13, 0, 0, 0, None, None, r, None) == -22
    assert L.bsdb_dev_find_duplicates_fixed(None, None, 0, 0, 0, 0, None, None, r, None) == -22
    assert L.bsdb_dev_find_duplicates_var(None, None, 0, None, 0, 0, 0, None, None, r, None) == -22
    assert L.bsdb_dev_find_duplicates_sig(None, None, 0, 0, None, r, None) == -22
    assert L.bsdb_dev_classify_pairs_fixed(None, None, 13, 0, None, 0, None, None) == -22
    assert L.bsdb_dev_classify_pairs_var(None, None, 0, None, 0, None, 0, None, None) == -22
    assert L.bsdb_find_duplicates_fixed(None, None, 13, 0, 0, None, None, r) == -22
    assert L.bsdb_find_duplicates_var(None, None, None, 0, 0, None, None, r) == -22
    assert L.bsdb_builder_find_duplicates(None, 0, None, None, r) == -22
    assert L.bsdb_kv_find_duplicates(None, b"/nonexistent/kv.db", 1, 0, 4096, 1, 0, None, None, r) == -22
    assert list(rep) == [9, 9, 9, 9]  # nothing was written


def test_report_dict():
    import numpy as np
    import bsdb_amd.native as N
    pairs = np.array([[7, 9], [2, 5], [2, 3], [0, 0]], np.uint64)
    kinds = np.array([1, 0, 2, 9], np.uint8)
    rep = N._dup_report(pairs, kinds, [3, 1, N.DUP_PARTIAL, 100])
    assert rep["pairs"].tolist() == [[2, 3], [2, 5], [7, 9]] and rep["kinds"].tolist() == [2, 0, 1]  # sorted together
    assert (rep["found"], rep["collisions"], rep["list_full"], rep["partial"], rep["keys"]) == (3, 1, False, True, 100)
    full = N._dup_report(pairs[:2], kinds[:2], [10, 0, N.DUP_LIST_FULL, 50])
    assert full["pairs"].shape == (2, 2) and full["list_full"] and full["found"] == 10
    none = N._dup_report(pairs[:0], kinds[:0], [0, 0, 0, 0])
    assert none["pairs"].shape == (0, 2) and none["found"] == 0


def test_duplicate_key_error_is_a_bsdb_error_with_code_minus_17():
    import bsdb_amd.native as N
    assert issubclass(N.DuplicateKeyError, N.BsdbError)
    rep = {"found": 2, "collisions": 0}
    e = N.DuplicateKeyError("bsdb_mph_build_var", rep, [b"k1", b"k2"])
    assert e.code == -17 == N.BSDB_EDUP and e.report is rep and e.keys == [b"k1", b"k2"]
    assert "EDUP" in str(e) and "2 duplicate pair" in str(e) and "k1" in str(e)
    with pytest.raises(N.BsdbError) as caught:  # code that catches BsdbError and checks .code keeps working
        raise e
    assert caught.value.code == -17
    import bsdb_amd.writer as W
    assert W.DuplicateKeyError is N.DuplicateKeyError


def test_java_native_shim_and_header_agree():
    java = _strip(open(os.path.join(ROOT, "jni", "GpuBuild.java")).read())
    m = re.search(r"public\s+static\s+native\s+void\s+kvFindDuplicates\s*\(([^)]*)\)\s*;", java, re.S)
    assert m
    jargs = _split_args(m.group(1))
    assert [a.split()[0] for a in jargs[-3:]] == ["long[]", "byte[]", "long[]"]
    shim = _strip(open(os.path.join(ROOT, "jni", "gpu_jni.c")).read())
    d = re.search(r"JNIEXPORT\s+void\s+JF\(kvFindDuplicates\)\s*\(([^)]*)\)\s*\{", shim, re.S)
    assert d and len(_split_args(d.group(1))) == len(jargs) + 2  # JNIEnv *, jclass, then the Java parameters
    body = shim[d.end():]
    call = re.search(r"bsdb_kv_find_duplicates\s*\(", body)
    assert call
    depth, j = 1, call.end()
    while depth:
        depth += {"(": 1, ")": -1}.get(body[j], 0)
        j += 1
    assert len(_split_args(body[call.end(): j - 1])) == len(_header_args("bsdb_kv_find_duplicates")) == 10
    # ctx, kv_base .. threads are the Java parameters; cap comes from the arrays' lengths
    assert len(jargs) == 9
    assert "utf(env, kv)" in body and "unutf(env, kv, k)" in body and "CHECK(rc)" in body
    assert "BSDB_DUP_WORDS" in body and "free(pairs)" in body
    strerror = open(os.path.join(ROOT, "bsdb_amd", "csrc", "bsdb_capi.hip")).read()
    msg = re.search(r'EDUP_MESSAGE\s*=\s*"([^"]+)"', java).group(1)
    assert f'case BSDB_EDUP: return "{msg}";' in strerror  # what the shim's IOException carries
    writer = _strip(open(os.path.join(ROOT, "jni", "GpuBSDBWriter.java")).read())
    assert "GpuBuild.kvFindDuplicates(" in writer and "GpuBuild.EDUP_MESSAGE" in writer
    assert re.search(r"new\s+IllegalStateException\s*\(\s*msg\s*,\s*cause\s*\)", writer)
    assert "report[0]" in writer and "Long.toHexString(pairs[" in writer  # the pair count and the first addresses

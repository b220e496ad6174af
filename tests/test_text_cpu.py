"""The text front end without a GPU: the header declares it, the library
exports it under ABI 6, the Python binding covers it, bad arguments are refused
before any device call, bsdb_text_max_records is bytes / 4 + 1, and the Python
driver (bsdb_amd.builder) resolves its inputs as documented."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "bsdb_mi355x.h")
NEW = ["bsdb_text_max_records", "bsdb_dev_text_split", "bsdb_dev_text_pack", "bsdb_builder_add_dev_var",
       "bsdb_text_set_chunk", "bsdb_text_build"]
EINVAL = -22


@pytest.fixture(scope="module")
def L():
    import bsdb_amd.native as N
    return N.lib()


def test_header_exports_and_abi(L):
    txt = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    declared = set(re.findall(r"\b(bsdb_\w+)\s*\(", txt))
    import bsdb_amd.native as N
    bound = {n for n, _, _ in N.SIGNATURES}
    for name in NEW:
        assert name in declared and name in bound and hasattr(L, name), name
    assert "#define BSDB_ABI_VERSION 6" in txt and L.bsdb_abi_version() == 6    # additive: the ABI number stays
    assert "#define BSDB_TEXT_WORDS 10" in txt and N.TEXT_WORDS == 10 and len(N.TEXT_FIELDS) == 10
    assert N.TEXT_FIELDS == ("lines", "records", "not_two_fields", "empty_key", "too_large", "key_bytes", "value_bytes",
                             "max_key_len", "max_value_len", "chunks")


def test_max_records(L):
    from bsdb_amd.native import text_max_records
    for b in (0, 1, 3, 4, 5, 15, 16, 17, 1 << 20, (1 << 32) - 1):
        assert text_max_records(b) == b // 4 + 1


def test_null_and_bad_arguments(L):
    rep = (C.c_uint64 * 10)()
    h = C.c_void_p()
    buf = (C.c_uint8 * 64)()
    p = C.addressof(buf)
    # no context
    assert L.bsdb_dev_text_split(None, p, 16, 32, 5, p, p, p, p, p, None) == EINVAL
    assert L.bsdb_dev_text_pack(None, p, 16, p, p, p, p, 1, 1, p, p, 64, p, p, p, 64, p, None, None, None, None) == EINVAL
    assert L.bsdb_builder_add_dev_var(None, p, p, 1, p, None, None, None) == EINVAL
    assert L.bsdb_text_set_chunk(None, 1 << 20) == EINVAL
    paths = (C.c_char_p * 1)(b"/nonexistent")
    assert L.bsdb_text_build(None, paths, 1, 32, b"/tmp/kv.db", 1, 4, 0, b"/tmp/i", b"/tmp/ia", rep, C.byref(h)) == EINVAL
    assert not h.value


def test_separator_must_be_one_ascii_byte():
    from bsdb_amd.native import Context
    assert Context._sep(" ") == 32 and Context._sep(b"\t") == 9 and Context._sep(",") == 44
    for bad in ("", "ab", b"::"):
        with pytest.raises(ValueError):
            Context._sep(bad)


def test_input_files(tmp_path):
    from bsdb_amd.builder import input_files
    d = tmp_path / "in"
    d.mkdir()
    for name in ("b.txt", "a.txt", "c.csv", "10.txt", "2.txt"):
        (d / name).write_bytes(b"k v\n")
    assert input_files(str(d)) == [str(d / n) for n in ("10.txt", "2.txt", "a.txt", "b.txt")]   # *.txt, by name
    assert input_files(str(d / "c.csv")) == [str(d / "c.csv")]                                  # a file as it is
    assert input_files([str(d / "b.txt"), str(d / "a.txt")]) == [str(d / "b.txt"), str(d / "a.txt")]  # in the order given
    for z in ("x.gz", "x.zstd"):
        with pytest.raises(NotImplementedError):
            input_files(str(d / z))
        with pytest.raises(NotImplementedError):
            input_files([str(d / "a.txt"), str(d / z)])


def test_cli_help_names_the_layout():
    r = subprocess.run([sys.executable, "-m", "bsdb_amd.builder", "-h"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-1000:]
    out = " ".join(r.stdout.split())
    assert "always the compact one" in out
    for flag in ("-i", "-o", "-s", "-cb", "-a", "-v", "-p"):
        assert re.search(rf"(^|[\s\[]){re.escape(flag)}\b", r.stdout), flag

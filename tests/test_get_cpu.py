"""The batched get's C ABI and bindings without a device: what the header
declares, the status and report constants in the header's order, and argument
errors before any device call."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "bsdb_mi355x.h")
FUNCS = ["bsdb_db_open", "bsdb_db_info", "bsdb_db_set_batch", "bsdb_db_get_fixed", "bsdb_db_get_var", "bsdb_db_free",
         "bsdb_dev_db_locate_fixed", "bsdb_dev_db_locate_var", "bsdb_dev_db_gather"]
STATUS = {"FOUND": 0, "REJECTED": 1, "KEY_MISMATCH": 2, "BAD_ADDR": 3}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)


def test_header_declares_the_functions_and_the_constants():
    h = _header()
    for f in FUNCS:
        assert re.search(r"\bint\s+" + f + r"\s*\(", h), f
    assert re.search(r"typedef\s+struct\s+bsdb_db\s+bsdb_db\s*;", h)
    assert re.search(r"#define\s+BSDB_GET_WORDS\s+6\b", h)
    assert re.search(r"#define\s+BSDB_DB_INFO_WORDS\s+8\b", h)
    for name, v in STATUS.items():
        assert re.search(rf"#define\s+BSDB_GET_{name}\s+{v}\b", h), name
    assert re.search(r"#define\s+BSDB_ABI_VERSION\s+6\b", h)  # additive: the ABI number stays
    import bsdb_amd.native as N
    assert N.lib().bsdb_abi_version() == 6
    # the handle list of the header's opening comment names the new handle
    top = open(HDR).read()
    top = top[top.index("Object handles"): top.index("#ifndef BSDB_MI355X_H")]
    assert re.search(r"^\s*\*\s+bsdb_db\s+\S", top, re.M)
    assert "out of scope" in open(HDR).read()[open(HDR).read().index("Batched get"):]


def test_constants_follow_the_header():
    import bsdb_amd.native as N
    assert (N.GET_FOUND, N.GET_REJECTED, N.GET_KEY_MISMATCH, N.GET_BAD_ADDR) == (0, 1, 2, 3)
    assert N.BSDB_E2BIG == -7 and re.search(r"#define\s+BSDB_E2BIG\s+\(-7\)", _header())
    txt = open(HDR).read()
    doc = txt[txt.index("The report is uint64_t[BSDB_GET_WORDS]"):]
    doc = doc[: doc.index("bsdb_dev_db_locate_*:")]
    words = {int(m.group(1)): m.group(2) for m in re.finditer(r"\[(\d)\]\s+([a-z_]+)", doc)}
    assert words == dict(enumerate(N.GET_FIELDS))
    assert N.GET_WORDS == 6 == len(N.GET_FIELDS)
    rep = N._get_report(range(10, 16))
    assert list(rep) == list(N.GET_FIELDS) and list(rep.values()) == list(range(10, 16))
    assert N.DB_INFO_WORDS == 8 == len(N.DB_INFO_FIELDS)
    from bsdb_amd import BSDBReader, Database  # re-exported
    assert BSDBReader.get and Database.get_fixed and Database.get_var and N.Mph.open_db


def test_null_arguments_are_einval_without_a_device():
    """NULL db / MPHF / out / keys: -22 before any device call (this runs where no GPU is), nothing written."""
    import bsdb_amd.native as N
    L = N.lib()
    out = C.c_void_p(0x1234)
    p = b"/nonexistent/index.db"
    kv = b"/nonexistent/kv.db"
    assert L.bsdb_db_open(None, kv, 1, 0, 4096, 0, p, C.byref(out)) == -22
    assert L.bsdb_db_open(None, kv, 1, 0, 4096, 0, p, None) == -22
    assert L.bsdb_db_open(None, None, 0, 0, 0, 1, p, C.byref(out)) == -22
    assert out.value == 0x1234  # nothing was written
    words = (C.c_uint64 * 8)(*([7] * 8))
    voff = (C.c_uint64 * 4)(*([7] * 4))
    status = (C.c_uint8 * 4)(*([7] * 4))
    values = (C.c_uint8 * 64)(*([7] * 64))
    keys = (C.c_uint8 * 64)()
    off = (C.c_uint64 * 4)(0, 1, 2, 3)
    a = C.addressof
    assert L.bsdb_db_info(None, a(words)) == -22
    assert L.bsdb_db_set_batch(None, 1000) == -22
    assert L.bsdb_db_free(None) == -22
    assert L.bsdb_db_get_fixed(None, a(keys), 13, 3, 64, a(values), a(voff), a(status), a(words)) == -22
    assert L.bsdb_db_get_fixed(None, None, 13, 3, 64, a(values), a(voff), a(status), a(words)) == -22
    assert L.bsdb_db_get_fixed(None, a(keys), 0, 3, 64, a(values), a(voff), a(status), a(words)) == -22
    assert L.bsdb_db_get_var(None, a(keys), a(off), 3, 64, a(values), a(voff), a(status), a(words)) == -22
    assert L.bsdb_db_get_var(None, None, None, 3, 64, None, None, None, None) == -22
    assert L.bsdb_dev_db_locate_fixed(None, a(keys), 13, 3, a(voff), a(voff), a(status), a(words), None) == -22
    assert L.bsdb_dev_db_locate_fixed(None, None, 13, 0, None, None, None, None, None) == -22
    assert L.bsdb_dev_db_locate_var(None, a(keys), 64, a(off), 3, a(voff), a(voff), a(status), a(words), None) == -22
    assert L.bsdb_dev_db_gather(None, a(voff), a(voff), 3, a(values), 64, None) == -22
    assert list(words) == [7] * 8 and list(voff) == [7] * 4 and list(status) == [7] * 4 and list(values) == [7] * 64

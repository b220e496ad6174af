"""The check of a database against text input: its C ABI, bindings and command
line without a device -- what the header declares, the status and report
constants in the header's order, the ABI number, argument errors before any
device call, and the parser's new flags beside the old ones' defaults."""
import ctypes as C
import fnmatch
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "bsdb_mi355x.h")
FUNCS = {"bsdb_dev_db_check": 12, "bsdb_db_check_text": 11}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)


def _arity(name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", _header(), re.S)
    assert m, name
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_header_declares_the_functions_and_the_constants():
    h = _header()
    for f, n in FUNCS.items():
        assert _arity(f) == n, f
    assert re.search(r"#define\s+BSDB_CHECK_WORDS\s+8\b", h)
    assert re.search(r"#define\s+BSDB_CHECK_VALUE_LEN\s+4\b", h)
    assert re.search(r"#define\s+BSDB_CHECK_VALUE_BYTES\s+5\b", h)
    assert re.search(r"#define\s+BSDB_ABI_VERSION\s+6\b", h)  # additive: the ABI number stays
    import bsdb_amd.native as N
    assert N.lib().bsdb_abi_version() == 6
    # the report's words in the specification comment are the binding's, in order
    txt = open(HDR).read()
    doc = txt[txt.index("The report is uint64_t[BSDB_CHECK_WORDS]"):]
    doc = doc[: doc.index("bsdb_dev_db_check:")]
    words = {int(m.group(1)): m.group(2) for m in re.finditer(r"\[(\d)\]\s+([a-z_]+)", doc)}
    assert words == dict(enumerate(N.CHECK_FIELDS))
    assert N.CHECK_WORDS == 8 == len(N.CHECK_FIELDS)
    assert (N.CHECK_OK, N.GET_REJECTED, N.GET_KEY_MISMATCH, N.GET_BAD_ADDR, N.CHECK_VALUE_LEN, N.CHECK_VALUE_BYTES) == tuple(range(6))
    assert N.CHECK_STATUS_NAMES == N.CHECK_FIELDS[1:7] and N.CHECK_NONE == 2**64 - 1
    rep = N._check_report([3, 1, 0, 0, 0, 1, 1, -1])  # (a torch int64 report holds first_bad = UINT64_MAX as -1)
    assert list(rep) == list(N.CHECK_FIELDS) and rep["first_bad"] == N.CHECK_NONE and rep["records"] == 3


def test_exports_and_signatures_carry_the_functions():
    import bsdb_amd.native as N
    sigs = {name: args for name, _, args in N.SIGNATURES}
    patterns = re.findall(r"global:\s*([^;]+);", open(os.path.join(ROOT, "bsdb_amd", "csrc", "exports.map")).read())
    for f, n in FUNCS.items():
        assert len(sigs[f]) == n == _arity(f), f
        assert any(fnmatch.fnmatchcase(f, p.strip()) for p in patterns), f      # the version script exports it
        assert getattr(N.lib(), f)                                                # and the library has it
    assert N.Database.check_text and N.Context.db_check and N.Context.check_report
    # the stage is a file of its own, included like the others; the kernels and the plan have theirs
    capi = open(os.path.join(ROOT, "bsdb_amd", "csrc", "bsdb_capi.hip")).read()
    assert '#include "capi_check.hip"' in capi and '#include "check_kernels.hip"' in capi
    assert '#include "check_plan.hpp"' in open(os.path.join(ROOT, "bsdb_amd", "csrc", "check_kernels.hip")).read()


def test_bad_arguments_are_einval_without_a_device():
    """NULL, misaligned or oversized arguments: -22 before any device call (this runs where no GPU is) and before the
    db is looked at -- the handle below is no database -- with nothing written."""
    import bsdb_amd.native as N
    L = N.lib()
    a = C.addressof
    fake = (C.c_uint64 * 64)()                # a non-NULL db handle the argument checks never read
    buf = (C.c_uint64 * 64)(*([7] * 64))      # 16-byte aligned below: ctypes arrays of u64 are 8-aligned, so align by hand
    base = (a(buf) + 15) & ~15
    status = (C.c_uint8 * 8)(*([7] * 8))
    report = (C.c_uint64 * 8)(*([7] * 8))

    def dev(db=a(fake), text=base, nbytes=64, vpos=base + 64, vlen=base + 96, src=base + 128, dbvlen=base + 192,
            st=a(status), count=4, rep=a(report)):
        return L.bsdb_dev_db_check(db, text, nbytes, vpos, vlen, src, dbvlen, st, count, 0, rep, None)

    assert dev(db=None) == -22
    assert dev(rep=None) == -22 and dev(rep=a(report) + 4) == -22
    assert dev(text=None) == -22 and dev(text=base + 8) == -22            # the text is 16-byte aligned
    assert dev(nbytes=1 << 32) == -22 and dev(nbytes=(1 << 64) - 1) == -22
    for name in ("vpos", "vlen", "src", "dbvlen", "st"):
        assert dev(**{name: None}) == -22, name
    for name in ("vpos", "vlen", "dbvlen"):
        assert dev(**{name: base + 66}) == -22, name                        # u32 arrays
    assert dev(src=base + 132) == -22                                       # a u64 array
    assert list(status) == [7] * 8 and list(report) == [7] * 8 and list(buf) == [7] * 64 and not any(fake)

    paths = (C.c_char_p * 2)(b"/nonexistent/a.txt", b"/nonexistent/b.txt")
    text_rep = (C.c_uint64 * 10)(*([7] * 10))
    bfile, boff, bst = (C.c_uint32 * 4)(), (C.c_uint64 * 4)(), (C.c_uint8 * 4)()
    n_bad = C.c_uint64(7)

    def host(db=a(fake), p=paths, nfiles=2, sep=32, trep=a(text_rep), crep=a(report), cap=4, f=a(bfile), o=a(boff), s=a(bst),
             nb=C.byref(n_bad)):
        return L.bsdb_db_check_text(db, p, nfiles, sep, trep, crep, cap, f, o, s, nb)

    assert host(db=None) == -22
    assert host(p=None) == -22 and host(nfiles=-1) == -22
    assert host(sep=10) == -22 and host(sep=13) == -22 and host(sep=128) == -22 and host(sep=-1) == -22
    assert host(trep=None) == -22 and host(crep=None) == -22 and host(nb=None) == -22
    assert host(f=None) == -22 and host(o=None) == -22 and host(s=None) == -22
    assert host(p=(C.c_char_p * 2)(b"/nonexistent/a.txt", None)) == -22
    assert list(text_rep) == [7] * 10 and list(report) == [7] * 8 and n_bad.value == 7


def test_parser_accepts_the_new_flags_and_keeps_the_old_defaults():
    from bsdb_amd import builder as B
    p = B.parser()
    a = p.parse_args(["-i", "in.txt"])
    assert (a.verify, a.verify_values, a.check) == (False, False, False)
    assert (a.output, a.separator, a.checksum_bits, a.approximate, a.partitions, a.layout, a.block_size, a.quiet) == \
        ("./rdb/", " ", 4, False, 8, "compact", 4096, False)
    a = p.parse_args(["-i", "in.txt", "-v"])
    assert (a.verify, a.verify_values, a.check) == (True, False, False)      # -v keeps its meaning
    a = p.parse_args(["-i", "in.txt", "-vv"])
    assert (a.verify, a.verify_values, a.check) == (False, True, False)
    a = p.parse_args(["-i", "in.txt", "--verify-values", "-v"])
    assert (a.verify, a.verify_values) == (True, True)
    a = p.parse_args(["--check", "-i", "a.txt", "-i", "b.txt", "-o", "db", "-s", ","])
    assert (a.check, a.input, a.output, a.separator, a.verify_values) == (True, ["a.txt", "b.txt"], "db", ",", False)
    import inspect
    sig = inspect.signature(B.build_text)
    assert sig.parameters["verify_values"].default is False and sig.parameters["verify"].default is False
    assert list(inspect.signature(B.check_text).parameters)[:4] == ["inputs", "db_dir", "separator", "device"]
    res = {"check": dict(zip(("records", "ok", "rejected", "key_mismatch", "bad_addr", "value_len", "value_bytes", "first_bad"),
                             (3, 1, 0, 0, 0, 1, 1, 1))), "bad": [("a.txt", 10, 4), ("b.txt", 0, 5)], "db_records": 3,
           "complete": False}
    assert B.format_check(res).splitlines() == [
        "records=3 ok=1 rejected=0 key_mismatch=0 bad_addr=0 value_len=1 value_bytes=1 db_records=3 complete=false",
        "a.txt:10 value_len", "b.txt:0 value_bytes"]

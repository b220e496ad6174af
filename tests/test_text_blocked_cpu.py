"""The blocked layout of the text front end without a GPU: the header declares
the three new entry points, the library exports them under ABI 6, the Python
binding covers them, NULL and bad arguments are refused before any device call,
bsdb_text_image_max is the plan's bound, and the command line parses the layout
flags with "compact" as the default."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "bsdb_mi355x.h")
NEW = ["bsdb_text_image_max", "bsdb_dev_text_pack_blocked", "bsdb_text_build_layout"]
EINVAL = -22


@pytest.fixture(scope="module")
def L():
    import bsdb_amd.native as N
    return N.lib()


def test_header_exports_and_abi(L):
    raw = open(HDR).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(bsdb_\w+)\s*\(", txt))
    import bsdb_amd.native as N
    bound = {n for n, _, _ in N.SIGNATURES}
    for name in NEW:
        assert name in declared and name in bound and hasattr(L, name), name
    assert "#define BSDB_ABI_VERSION 6" in txt and L.bsdb_abi_version() == 6    # additive: the ABI number stays
    assert "DEVIATION 6" in raw and "BlockedKVWriter.java:45-74" in raw         # the rule and its one deviation


def test_null_and_bad_arguments(L):
    rep = (C.c_uint64 * 10)()
    h = C.c_void_p()
    buf = (C.c_uint8 * 64)()
    p = C.addressof(buf)
    # no context: refused whatever else is given
    assert L.bsdb_dev_text_pack_blocked(None, p, 16, p, p, p, p, 1, 1, 4096, p, p, 64, p, p, p, 64, p, None, None, None,
                                        None) == EINVAL
    paths = (C.c_char_p * 1)(b"/nonexistent")
    assert L.bsdb_text_build_layout(None, paths, 1, 32, b"/tmp/kv.db", 1, 1, 4096, 4, 0, b"/tmp/i", b"/tmp/ia", rep,
                                    C.byref(h)) == EINVAL
    assert not h.value
    # with a context that is only an address (never dereferenced: the arguments are checked first)
    fake = C.addressof((C.c_uint8 * 16)())
    for fmt, bs in ((2, 4096), (-1, 4096), (1, 0), (1, 4095), (1, 6000), (1, 69632)):
        assert L.bsdb_text_build_layout(fake, paths, 1, 32, b"/tmp/kv.db", 1, fmt, bs, 4, 0, b"/tmp/i", b"/tmp/ia", rep,
                                        C.byref(h)) == EINVAL, (fmt, bs)
    sizes = (C.c_uint64 * 1)(0)
    runs = (C.c_uint64 * 1)(77)
    text = (C.c_uint8 * 64)()
    tp = (C.addressof(text) + 15) & ~15
    for bs in (0, 4095, 6000, 69632):
        assert L.bsdb_dev_text_pack_blocked(fake, tp, 16, p, p, p, p, 1, 1, bs, sizes, p, 64, runs, None, None, 0, None, None,
                                            None, None, None) == EINVAL, bs
    for before in (1, 4095, 4097, (1 << 44) + 4096):                            # F: a multiple of 4096, below 2^44
        sizes[0] = before
        assert L.bsdb_dev_text_pack_blocked(fake, tp, 16, p, p, p, p, 1, 1, 4096, sizes, p, 64, runs, None, None, 0, None,
                                            None, None, None, None) == EINVAL, before
    assert runs[0] == 77                                                        # nothing was written


def test_image_max_matches_the_plan(L):
    from bsdb_amd.native import text_image_max
    for b in (0, 1, 4, 4096, 1 << 20, (1 << 32) - 1):
        assert text_image_max(b) == b + b // 2 + 16                             # format 0: as before
        assert L.bsdb_text_image_max(b, 8, 0, 12345) == b + b // 2 + 16
        for parts in (1, 3, 128):
            for bs in (4096, 8192, 65536):
                want = 2 * (b + b // 4 + 2) + parts * bs + 16
                assert text_image_max(b, parts, 1, bs) == want
                assert want >= b + b // 2 + 16
    # the bound on the worst small case: every block holds one record of B / 2 + 1 bytes
    n, bs = 100, 4096
    size = bs // 2 + 1
    assert n * bs <= text_image_max(n * (size - 1), 1, 1, bs)


def test_command_line_flags():
    from bsdb_amd.builder import LAYOUTS, parser
    ap = parser()
    a = ap.parse_args(["-i", "x"])
    assert a.layout == "compact" and a.block_size == 4096                       # existing callers depend on it
    a = ap.parse_args(["-i", "x", "-l", "blocked", "-bs", "8192"])
    assert a.layout == "blocked" and a.block_size == 8192
    a = ap.parse_args(["-i", "x", "--layout", "blocked", "--block-size", "65536"])
    assert a.layout == "blocked" and a.block_size == 65536
    with pytest.raises(SystemExit):
        ap.parse_args(["-i", "x", "-l", "compressed"])
    assert LAYOUTS == {"compact": 0, "blocked": 1}
    assert "reference's own default is blocked" in " ".join(ap.format_help().split())


def test_build_text_refuses_an_unknown_layout(tmp_path):
    from bsdb_amd.builder import build_text
    with pytest.raises(ValueError):
        build_text(str(tmp_path / "in.txt"), str(tmp_path / "db"), layout="compressed")

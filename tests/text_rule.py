"""The record rule of the text front end restated in plain Python, for the
text tests (not a test module).  Lines are ``bytes.splitlines()`` (which ends a
line at "\\n", "\\r" and "\\r\\n" only), fields ``line.split(sep)`` with the
trailing empty fields dropped (String.split), a record a line with exactly two
fields; then the empty-key and size tests.  Nothing here shares a method with
the library's position lists."""
import numpy as np

MAX_KEY, MAX_VALUE = 255, 32510
FIELDS = ("lines", "records", "not_two_fields", "empty_key", "too_large", "key_bytes", "value_bytes", "max_key_len",
          "max_value_len")


def verdict(line: bytes, sep: bytes):
    """(class, key, value) of one line without its terminator."""
    f = line.split(sep)
    while f and f[-1] == b"":
        f.pop()
    if len(f) != 2:
        return "not_two_fields", None, None
    k, v = f
    if len(k) == 0:
        return "empty_key", None, None
    if len(k) > MAX_KEY or len(v) > MAX_VALUE:
        return "too_large", None, None
    return "records", k, v


def restate(text: bytes, sep: bytes):
    """(records, report): records = [(kpos, key, vpos, value)] in input order,
    report = the first nine words of the library's report as a dict."""
    rep = dict.fromkeys(FIELDS, 0)
    recs = []
    pos = 0
    for full in text.splitlines(keepends=True):
        line = full.rstrip(b"\r\n") if full[-1:] in (b"\n", b"\r") else full
        # (a line's own bytes hold no terminator, so rstrip takes its terminator only)
        assert len(full) - len(line) in (0, 1, 2)
        cls, k, v = verdict(line, sep)
        rep["lines"] += 1
        rep[cls] += 1
        if cls == "records":
            recs.append((pos, k, pos + len(k) + 1, v))
            rep["key_bytes"] += len(k)
            rep["value_bytes"] += len(v)
            rep["max_key_len"] = max(rep["max_key_len"], len(k))
            rep["max_value_len"] = max(rep["max_value_len"], len(v))
        pos += len(full)
    assert pos == len(text) and rep["lines"] == len(text.splitlines())
    return recs, rep


def image_of(recs):
    """The compact kv.db bytes of the records, back to back, and each record's offset."""
    out, offs = bytearray(), []
    for _, k, _, v in recs:
        offs.append(len(out))
        out += bytes([len(k), len(v) >> 8, len(v) & 0xFF]) + k + v
    return bytes(out), offs


def run_bounds(k: int, parts: int):
    return [p * k // parts for p in range(parts + 1)]


def value_heads(recs):
    v8 = np.zeros(len(recs), np.uint64)
    vl = np.zeros(len(recs), np.uint8)
    for i, (_, _, _, v) in enumerate(recs):
        vl[i] = min(len(v), 8)
        v8[i] = int.from_bytes(v[:8].ljust(8, b"\0"), "little")
    return v8, vl

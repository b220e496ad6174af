"""Text files of ``key<sep>value`` lines into a database, on the device.

The reference's command-line ``Builder`` (tools/Builder.java:144-176) reads
its input files line by line, splits every line at the separator and puts the
lines that are records; ``build()`` then makes the hash and the index.  Here
the whole of that is one native call, ``bsdb_text_build_layout``: the text is
split into lines and fields, the records packed into the compact kv.db layout
(or, with ``layout="blocked"``, placed into the blocks of the reference's
default layout) and their keys handed to the streaming builder by gfx950
kernels (bsdb_amd/csrc/text_kernels.hip, text_blocked_kernels.hip).  There is
no CPU fallback for the parse.

``build_text`` writes the file set of ``bsdb_amd.writer.BSDBWriter``:
kv.db.<p>, config.properties, hash.dump, index.db, index_a.db.

The record rule and where it departs from the reference are in
include/bsdb_mi355x.h ("text front end") and DESIGN.md §3.7: keys of 0 bytes
are dropped, bytes are taken verbatim (no charset decoding), the separator is
one literal byte (never a regular expression), a line must fit one chunk.

Command line, mirroring ``Builder``'s flags::

    python -m bsdb_amd.builder -i INPUT [-i INPUT ...] -o OUT_DIR [-s SEP] [-cb BITS] [-a] [-v] [-vv] [-p PARTITIONS]
                               [-l {compact,blocked}] [-bs BLOCK_SIZE]
    python -m bsdb_amd.builder --check -i INPUT [-i INPUT ...] -o DB_DIR [-s SEP]

``-vv`` (``build_text(verify_values=True)``) is the reference's ``-v``
(tools/Builder.java:184-228): the input is read a second time and every
record's value is compared with what the database returns for its key, on the
device (``bsdb_db_check_text``, bsdb_amd/csrc/check_kernels.hip).  ``--check``
builds nothing and runs that comparison of an existing database directory
against text files (``check_text``).  Both exit with status 2 on a mismatch.
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import Optional

from .native import BSDB_EDUP, CHECK_STATUS_NAMES, BsdbError, Context, DuplicateKeyError
from .writer import VerifyError

COMPRESSED_SUFFIXES = (".gz", ".zstd", ".zst")


def input_files(inputs) -> list:
    """``inputs``: a file, a list of files, or a directory (its ``*.txt``
    files sorted by name).  Compressed inputs are not read."""
    if isinstance(inputs, (str, bytes, os.PathLike)):
        inputs = os.fspath(inputs)
        if os.path.isdir(inputs):
            files = [os.path.join(inputs, f) for f in sorted(os.listdir(inputs)) if f.endswith(".txt")]
        else:
            files = [inputs]
    else:
        files = [os.fspath(f) for f in inputs]
    for f in files:
        if str(f).endswith(COMPRESSED_SUFFIXES):
            raise NotImplementedError(f"{f}: compressed inputs are not read (out of scope)")
    return files


LAYOUTS = {"compact": 0, "blocked": 1}


def _write_config(out_dir: str, report: dict, approximate: bool, checksum_bits: int, layout: str = "compact",
                  block_size: int = 4096):
    """config.properties with the keys of BSDBWriter._write_config, the
    statistics taken from the text report.  The blocked layout's block size
    goes where BSDBReader reads it: kv.compress.block.size."""
    n = report["records"]
    blocked = layout == "blocked"
    props = {
        "kv.compressed": "false", "kv.compact": "false" if blocked else "true",
        "kv.compress.block.size": block_size if blocked else 8192,
        "index.approximate": str(bool(approximate)).lower(), "hash.checksum.bits": checksum_bits,
        "kv.count": n, "kv.key.len.max": report["max_key_len"],
        "kv.key.len.avg": report["key_bytes"] / n if n else 0.0, "kv.value.len.max": report["max_value_len"],
        "kv.value.len.avg": report["value_bytes"] / n if n else 0.0,
    }
    with open(os.path.join(out_dir, "config.properties"), "w") as f:
        for k, v in props.items():
            f.write(f"{k} = {v}\n")


def _duplicate_error(ctx: Context, kv_base: str, partitions: int, fmt: int = 0, block_size: int = 4096) -> DuplicateKeyError:
    """The duplicate finder over the kv.db files the failed build completed,
    with up to 16 colliding keys read back at the reported addresses (blocked:
    the block's page in bits 16-47, the offset in the low 16 bits)."""
    rep = ctx.kv_find_duplicates(kv_base, partitions, fmt, block_size)
    keys, seen = [], set()
    for addr in rep["pairs"].reshape(-1).tolist():
        p, off = int(addr) >> 56, int(addr) & ((1 << 56) - 1)
        if fmt == 1:
            off = ((int(addr) >> 16) & 0xFFFFFFFF) * 4096 + (int(addr) & 0xFFFF)
        with open(f"{kv_base}.{p}", "rb") as f:
            f.seek(off)
            head = f.read(3)
            if len(head) < 3:
                continue
            k = f.read(head[0])
        if k not in seen:
            seen.add(k)
            keys.append(k)
            if len(keys) == 16:
                break
    return DuplicateKeyError("bsdb_text_build", rep, keys)


def build_text(inputs, out_dir: str, separator=" ", checksum_bits: int = 4, approximate: bool = False,
               partitions: int = 8, verify: bool = False, device: int = 0, chunk_bytes: Optional[int] = None,
               layout: str = "compact", block_size: int = 4096, verify_values: bool = False) -> dict:
    """Builds the database of the records in ``inputs`` into ``out_dir`` and
    returns the text report (native.TEXT_FIELDS).  ``layout``: "compact" (the
    reference's -c) or "blocked" (the reference's default) in blocks of
    ``block_size`` bytes.  ``verify=True`` checks the
    finished files on the device (Mph.verify_kv) and raises VerifyError when
    they are not clean.  ``verify_values=True`` then opens the database on the
    MPHF just built and checks it against the same files, key -> value
    (Database.check_text; an approximate build's index_a.db too), and raises
    VerifyError carrying that dict when a record is not OK or the OK records
    are not all the text's; a clean check's dict is returned as
    ``report["values"]``.  A duplicate key raises DuplicateKeyError (``.keys``:
    up to 16 of them)."""
    if layout not in LAYOUTS:
        raise ValueError("layout is 'compact' or 'blocked'")
    fmt = LAYOUTS[layout]
    files = input_files(inputs)
    os.makedirs(out_dir, exist_ok=True)
    kv = os.path.join(out_dir, "kv.db")
    index, index_a = os.path.join(out_dir, "index.db"), os.path.join(out_dir, "index_a.db")
    with Context(device) as ctx:
        if chunk_bytes is not None:
            ctx.text_set_chunk(chunk_bytes)
        try:
            mph, report = ctx.text_build(files, separator, kv, partitions, checksum_bits, index, index_a, approximate,
                                         fmt=fmt, block_size=block_size)
        except BsdbError as e:
            if e.code != BSDB_EDUP:
                raise
            raise _duplicate_error(ctx, kv, partitions, fmt, block_size) from e
        try:
            _write_config(out_dir, report, approximate, checksum_bits, layout, block_size)
            mph.dump(os.path.join(out_dir, "hash.dump"))
            if verify:
                rep = mph.verify_kv(kv, partitions, index, index_a, approximate, fmt=fmt, block_size=block_size)
                if not rep["ok"]:
                    raise VerifyError(rep)
            if verify_values:
                for approx in ([False, True] if approximate else [False]):
                    with mph.open_db(kv, partitions, index_a if approx else index, approx, fmt, block_size) as db:
                        res = db.check_text(files, separator)
                    res["db_records"] = report["records"]
                    res["complete"] = res["check"]["ok"] == report["records"]
                    if not res["ok"] or not res["complete"]:
                        raise VerifyError(res)
                    report.setdefault("values", res)  # (the exact check's dict rides with the report)
        finally:
            mph.close()
    return report


def check_text(inputs, db_dir: str, separator=" ", device: int = 0, approximate: Optional[bool] = None,
               bad_cap: int = 16, strict: bool = False) -> dict:
    """Checks the database directory ``db_dir`` (opened as BSDBReader opens
    it: config.properties, hash.dump, the kv.db files) against the records of
    ``inputs``, key -> value, on the device.  Returns the dict of
    Database.check_text plus ``db_records`` (the database's record count) and
    ``complete``: the OK records are as many as the database holds, so the
    text is not only in the database but all of it (for inputs without a
    repeated key).  ``strict=True`` raises VerifyError carrying the dict when a
    record is not OK."""
    from .reader import BSDBReader
    files = input_files(inputs)
    with BSDBReader(db_dir, approximate=approximate, device=device) as r:
        res = r.db.check_text(files, separator, bad_cap)
        res["db_records"] = r.db.info()["n"]
    res["complete"] = res["check"]["ok"] == res["db_records"]
    if strict and not res["ok"]:
        raise VerifyError(res)
    return res


def format_check(res: dict) -> str:
    """The counts on one line, then ``path:offset status`` for the records held in ``bad``."""
    lines = [" ".join(f"{k}={v}" for k, v in res["check"].items() if k != "first_bad") +
             f" db_records={res['db_records']} complete={str(res['complete']).lower()}"]
    lines += [f"{path}:{off} {CHECK_STATUS_NAMES[st] if st < len(CHECK_STATUS_NAMES) else st}" for path, off, st in res["bad"]]
    return "\n".join(lines)


def parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(
        prog="python -m bsdb_amd.builder",
        description="Build a database from text files of key<separator>value lines on the GPU. "
                    "Without -l the kv.db layout is always the compact one (the reference's -c); "
                    "-l blocked writes the reference's default layout. "
                    "Compressed records (-z) and compressed inputs are not supported.")
    ap.add_argument("-i", "--input", action="append", required=True,
                    help="input file or directory (its *.txt files, sorted by name); may be given more than once")
    ap.add_argument("-o", "--output", default="./rdb/", help="output directory, default ./rdb/")
    ap.add_argument("-s", "--separator", default=" ", help="key/value separator, one literal byte, default space")
    ap.add_argument("-cb", "--checksum-bits", type=int, default=4, help="checksum bit length, default 4")
    ap.add_argument("-a", "--approximate", action="store_true", help="approximate mode: index_a.db holds the first 8 value bytes")
    ap.add_argument("-v", "--verify", action="store_true", help="verify the generated index on the device")
    ap.add_argument("-vv", "--verify-values", action="store_true",
                    help="after the build, read the input again and compare every record's value with what the "
                         "database returns for its key, on the device; exit status 2 on a mismatch")
    ap.add_argument("--check", action="store_true",
                    help="build nothing: check the database in -o against the input, key -> value; exit status 2 on a mismatch")
    ap.add_argument("-p", "--partitions", type=int, default=8, help="kv.db partition files, 1..128, default 8")
    ap.add_argument("-l", "--layout", choices=sorted(LAYOUTS), default="compact",
                    help="kv.db layout, default compact; the reference's own default is blocked")
    ap.add_argument("-bs", "--block-size", type=int, default=4096,
                    help="block bytes of the blocked layout: a multiple of 4096 up to 65536, default 4096")
    ap.add_argument("-q", "--quiet", action="store_true", help="print nothing")
    return ap


def main(argv=None) -> int:
    a = parser().parse_args(argv)
    files = []
    for i in a.input:
        files += input_files(i)
    if a.check:
        res = check_text(files, a.output, a.separator)
        if not a.quiet:
            print(format_check(res))
        return 0 if res["ok"] else 2
    try:
        report = build_text(files, a.output, a.separator, a.checksum_bits, a.approximate, a.partitions, a.verify,
                            layout=a.layout, block_size=a.block_size, verify_values=a.verify_values)
    except VerifyError as e:
        if "check" not in e.report:  # (-v's report: as before)
            raise
        if not a.quiet:
            print(format_check(e.report))
        return 2
    if not a.quiet:
        print(" ".join(f"{k}={v}" for k, v in report.items() if k != "values"))
        if "values" in report:
            print(format_check(report["values"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())

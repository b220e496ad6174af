"""Text files of ``key<sep>value`` lines into a database, on the device.

The reference's command-line ``Builder`` (tools/Builder.java:144-176) reads
its input files line by line, splits every line at the separator and puts the
lines that are records; ``build()`` then makes the hash and the index.  Here
the whole of that is one native call, ``bsdb_text_build``: the text is split
into lines and fields, the records packed into the compact kv.db layout and
their keys handed to the streaming builder by gfx950 kernels
(bsdb_amd/csrc/text_kernels.hip).  There is no CPU fallback for the parse.

``build_text`` writes the file set of ``bsdb_amd.writer.BSDBWriter``:
kv.db.<p>, config.properties, hash.dump, index.db, index_a.db.

The record rule and where it departs from the reference are in
include/bsdb_mi355x.h ("text front end") and DESIGN.md §3.7: keys of 0 bytes
are dropped, bytes are taken verbatim (no charset decoding), the separator is
one literal byte (never a regular expression), a line must fit one chunk.

Command line, mirroring ``Builder``'s flags::

    python -m bsdb_amd.builder -i INPUT [-i INPUT ...] -o OUT_DIR [-s SEP] [-cb BITS] [-a] [-v] [-p PARTITIONS]
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import Optional

from .native import BSDB_EDUP, BsdbError, Context, DuplicateKeyError
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


def _write_config(out_dir: str, report: dict, approximate: bool, checksum_bits: int):
    """config.properties with the keys of BSDBWriter._write_config, the
    statistics taken from the text report."""
    n = report["records"]
    props = {
        "kv.compressed": "false", "kv.compact": "true", "kv.compress.block.size": 8192,
        "index.approximate": str(bool(approximate)).lower(), "hash.checksum.bits": checksum_bits,
        "kv.count": n, "kv.key.len.max": report["max_key_len"],
        "kv.key.len.avg": report["key_bytes"] / n if n else 0.0, "kv.value.len.max": report["max_value_len"],
        "kv.value.len.avg": report["value_bytes"] / n if n else 0.0,
    }
    with open(os.path.join(out_dir, "config.properties"), "w") as f:
        for k, v in props.items():
            f.write(f"{k} = {v}\n")


def _duplicate_error(ctx: Context, kv_base: str, partitions: int) -> DuplicateKeyError:
    """The duplicate finder over the kv.db files the failed build completed,
    with up to 16 colliding keys read back at the reported addresses."""
    rep = ctx.kv_find_duplicates(kv_base, partitions)
    keys, seen = [], set()
    for addr in rep["pairs"].reshape(-1).tolist():
        p, off = int(addr) >> 56, int(addr) & ((1 << 56) - 1)
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
               partitions: int = 8, verify: bool = False, device: int = 0, chunk_bytes: Optional[int] = None) -> dict:
    """Builds the database of the records in ``inputs`` into ``out_dir`` and
    returns the text report (native.TEXT_FIELDS).  ``verify=True`` checks the
    finished files on the device (Mph.verify_kv) and raises VerifyError when
    they are not clean.  A duplicate key raises DuplicateKeyError (``.keys``:
    up to 16 of them)."""
    files = input_files(inputs)
    os.makedirs(out_dir, exist_ok=True)
    kv = os.path.join(out_dir, "kv.db")
    index, index_a = os.path.join(out_dir, "index.db"), os.path.join(out_dir, "index_a.db")
    with Context(device) as ctx:
        if chunk_bytes is not None:
            ctx.text_set_chunk(chunk_bytes)
        try:
            mph, report = ctx.text_build(files, separator, kv, partitions, checksum_bits, index, index_a, approximate)
        except BsdbError as e:
            if e.code != BSDB_EDUP:
                raise
            raise _duplicate_error(ctx, kv, partitions) from e
        try:
            _write_config(out_dir, report, approximate, checksum_bits)
            mph.dump(os.path.join(out_dir, "hash.dump"))
            if verify:
                rep = mph.verify_kv(kv, partitions, index, index_a, approximate)
                if not rep["ok"]:
                    raise VerifyError(rep)
        finally:
            mph.close()
    return report


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(
        prog="python -m bsdb_amd.builder",
        description="Build a database from text files of key<separator>value lines on the GPU. "
                    "The kv.db layout is always the compact one (the reference's -c); "
                    "compressed records (-z) and compressed inputs are not supported.")
    ap.add_argument("-i", "--input", action="append", required=True,
                    help="input file or directory (its *.txt files, sorted by name); may be given more than once")
    ap.add_argument("-o", "--output", default="./rdb/", help="output directory, default ./rdb/")
    ap.add_argument("-s", "--separator", default=" ", help="key/value separator, one literal byte, default space")
    ap.add_argument("-cb", "--checksum-bits", type=int, default=4, help="checksum bit length, default 4")
    ap.add_argument("-a", "--approximate", action="store_true", help="approximate mode: index_a.db holds the first 8 value bytes")
    ap.add_argument("-v", "--verify", action="store_true", help="verify the generated index on the device")
    ap.add_argument("-p", "--partitions", type=int, default=8, help="kv.db partition files, 1..128, default 8")
    ap.add_argument("-q", "--quiet", action="store_true", help="print nothing")
    a = ap.parse_args(argv)
    files = []
    for i in a.input:
        files += input_files(i)
    report = build_text(files, a.output, a.separator, a.checksum_bits, a.approximate, a.partitions, a.verify)
    if not a.quiet:
        print(" ".join(f"{k}={v}" for k, v in report.items()))
    return 0


if __name__ == "__main__":
    sys.exit(main())

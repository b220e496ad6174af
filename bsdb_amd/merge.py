"""A delta applied to a database directory, on the device (bsdb_db_merge):
yesterday's directory plus today's changes gives today's directory.  BASE_DIR,
and the optional delta and removed directories, are made resident on one
context; the output holds every record of the delta, and every record of the
base whose key neither the delta nor the removed directory holds (of the
removed directory only the keys matter).  No record passes through text, so
records that ``dump_text`` reports as NOT_TEXT are carried like any other.

    python -m bsdb_amd.merge BASE_DIR -o OUT_DIR [--delta DIR] [--removed DIR] [-p PARTITIONS]
                             [-l {compact,blocked}] [-bs BLOCK_SIZE] [-cb BITS] [-a] [-v]

Without --delta and --removed it is a rebuild of BASE_DIR's records into
another partition count, layout, checksum width or approximate mode.  Options
that are not given default to BASE_DIR's config.properties.  ``-v`` verifies
the finished files on the device (Mph.verify_kv).  It prints one line of
counts; exit status 0, or 2 when the merge stopped on a damaged input (a slot
whose address names no record): no index file is written then.  Exact
databases only; all inputs must fit the device together.  ``bsdb_amd.diff``
writes the delta as text, ``bsdb_amd.builder`` builds the small databases this
reads.
"""
from __future__ import annotations

import os
from typing import Optional

from .builder import LAYOUTS, _write_config
from .native import BSDB_EVERIFY, MERGE_FIELDS, BsdbError
from .reader import BSDBReader, _read_config
from .writer import VerifyError


def _same_dir(a: str, b: str) -> bool:
    return os.path.realpath(a) == os.path.realpath(b)


def merge_dirs(base_dir: str, out_dir: str, delta_dir: Optional[str] = None, removed_dir: Optional[str] = None,
               partitions: Optional[int] = None, layout: Optional[str] = None, block_size: Optional[int] = None,
               checksum_bits: Optional[int] = None, approximate: Optional[bool] = None, verify: bool = False,
               device: int = 0) -> dict:
    """Database.merge of the directories: the file set of ``build_text`` in
    `out_dir`.  Returns the merge report (native.MERGE_FIELDS).  A damaged
    input raises BsdbError (code BSDB_EVERIFY, the report in ``.merge_report``)
    and leaves no index file, config or hash.dump; ``verify=True`` raises
    VerifyError when the finished files are not clean."""
    inputs = [d for d in (base_dir, delta_dir, removed_dir) if d is not None]
    if any(_same_dir(out_dir, d) for d in inputs):
        raise ValueError("the output directory is one of the inputs")
    cfgs = [_read_config(os.path.join(d, "config.properties")) for d in inputs[: 1 + (delta_dir is not None)]]
    cfg = cfgs[0]
    if layout is None:
        layout = "compact" if cfg.get("kv.compact", "true").lower() == "true" else "blocked"
    if layout not in LAYOUTS:
        raise ValueError("layout is 'compact' or 'blocked'")
    if block_size is None:
        block_size = int(cfg.get("kv.compress.block.size", 4096)) if layout == "blocked" and cfg.get("kv.compact", "true").lower() != "true" else 4096
    if checksum_bits is None:
        checksum_bits = int(cfg.get("hash.checksum.bits", 4))
    if approximate is None:
        approximate = cfg.get("index.approximate", "false").lower() == "true"
    os.makedirs(out_dir, exist_ok=True)
    kv = os.path.join(out_dir, "kv.db")
    index, index_a = os.path.join(out_dir, "index.db"), os.path.join(out_dir, "index_a.db")
    with BSDBReader(base_dir, approximate=False, device=device) as base:
        if partitions is None:
            partitions = base.partitions
        others = []
        try:
            for d in (delta_dir, removed_dir):
                others.append(BSDBReader(d, approximate=False, ctx=base.ctx) if d is not None else None)
            delta, removed = others
            report, mph = base.db.merge(kv, partitions, checksum_bits, index, index_a if approximate else None, approximate,
                                        LAYOUTS[layout], block_size, delta.db if delta else None, removed.db if removed else None)
        finally:
            for r in others:
                if r is not None:
                    r.close()
        try:
            stats = {"records": report["out_records"], "key_bytes": report["out_key_bytes"], "value_bytes": report["out_value_bytes"],
                     "max_key_len": max(int(float(c.get("kv.key.len.max", 0))) for c in cfgs),
                     "max_value_len": max(int(float(c.get("kv.value.len.max", 0))) for c in cfgs)}
            _write_config(out_dir, stats, approximate, checksum_bits, layout, block_size)
            mph.dump(os.path.join(out_dir, "hash.dump"))
            if verify:
                rep = mph.verify_kv(kv, partitions, index, index_a, approximate, fmt=LAYOUTS[layout], block_size=block_size)
                if not rep["ok"]:
                    raise VerifyError(rep)
        finally:
            mph.close()
    return report


def format_report(report: dict) -> str:
    return "  ".join(f"{k} {report[k]}" for k in MERGE_FIELDS)


def main(argv=None) -> int:
    import argparse
    ap = argparse.ArgumentParser(prog="python -m bsdb_amd.merge",
                                 description="merge database directories on the device: delta over base, minus removed")
    ap.add_argument("base_dir", metavar="BASE_DIR", help="the database the merge starts from")
    ap.add_argument("-o", "--output", required=True, metavar="OUT_DIR", help="the directory to write (none of the inputs)")
    ap.add_argument("--delta", metavar="DIR", default=None, help="a database whose records replace or join the base's")
    ap.add_argument("--removed", metavar="DIR", default=None, help="a database whose keys leave the base")
    ap.add_argument("-p", "--partitions", type=int, default=None, help="kv.db partition files, 1..128 (default: the base's)")
    ap.add_argument("-l", "--layout", choices=sorted(LAYOUTS), default=None, help="kv.db layout (default: the base's)")
    ap.add_argument("-bs", "--block-size", type=int, default=None, help="block bytes of the blocked layout (default: the base's, or 4096)")
    ap.add_argument("-cb", "--checksum-bits", type=int, default=None, help="checksum bit length (default: the base's)")
    ap.add_argument("-a", "--approximate", action="store_true", default=None, help="also write index_a.db (default: as the base)")
    ap.add_argument("-v", "--verify", action="store_true", help="verify the finished files on the device")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    if any(_same_dir(a.output, d) for d in (a.base_dir, a.delta, a.removed) if d is not None):
        ap.error("OUT_DIR is one of the inputs")
    try:
        report = merge_dirs(a.base_dir, a.output, a.delta, a.removed, a.partitions, a.layout, a.block_size, a.checksum_bits,
                            a.approximate, a.verify, a.device)
    except BsdbError as e:
        if e.code != BSDB_EVERIFY or not hasattr(e, "merge_report"):
            raise
        print(format_report(e.merge_report) + "  stopped: damaged input")
        return 2
    print(format_report(report))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())

"""Host-side mirror of the reference's SyncReader
(src/main/java/tech/bsdb/read/SyncReader.java, getAsBytes :44-57) over the
batched get of the C ABI (bsdb_db_*): the database directory a BSDBWriter left
is made resident on one device and read a batch of keys at a time.

``BSDBReader(base_path)`` reads ``config.properties`` as
``BSDBWriter._write_config`` writes it (kv.compact, kv.compress.block.size,
index.approximate), counts the ``kv.db.<p>`` files and loads ``hash.dump``
(GOV.dump's raw layout, which carries no checksum bits: an absent key is then
told from a present one by the key compare alone, and in approximate mode
every absent key whose rank is below n is a false positive, as for the
reference without checksum bits).  Compressed kv.db files are out of scope, as
for the scan.  Every lookup runs in the gfx950 kernels: no CPU fallback.

An exact database also lists itself, by slot (bsdb_db_scan, bsdb_db_dump_text):
``items()`` yields its (key, value) pairs, ``dump_text(path)`` writes them as
``key<sep>value`` lines that ``BSDBWriter.build_text`` reads back, and

    python -m bsdb_amd.reader --dump out.txt -d DB [-s SEP] [--first N --count M]

does the latter from the command line: exit status 0 when every slot is OK, 2
when a slot's address names no record or a record's line does not read back.

Two exact databases on one device context are compared on the device
(bsdb_db_diff): ``BSDBReader(b_dir, ctx=a.ctx)`` borrows the context of reader
``a`` and does not close it, and ``a.diff(b, upsert=..., removed=...)`` gives
the counts of both directions and the delta as text (bsdb_amd/diff.py is its
command line).
"""
from __future__ import annotations

import os
from typing import Optional

import numpy as np

from .native import GET_FOUND, SCAN_NONE, SCAN_OK, Context, Database


def _read_config(path: str) -> dict:
    props = {}
    with open(path) as f:
        for line in f:
            line = line.strip()
            if not line or line[0] in "#!" or "=" not in line:
                continue
            k, v = line.split("=", 1)
            props[k.strip()] = v.strip()
    return props


class BSDBReader:
    def __init__(self, base_path: str, approximate: Optional[bool] = None, device: int = 0, ctx: Optional[Context] = None):
        cfg = _read_config(os.path.join(base_path, "config.properties"))
        if cfg.get("kv.compressed", "false").lower() == "true":
            raise NotImplementedError("compressed kv.db files are not read (the zstd layout is out of scope)")
        compact = cfg.get("kv.compact", "true").lower() == "true"
        block_size = int(cfg.get("kv.compress.block.size", 4096))
        if approximate is None:
            approximate = cfg.get("index.approximate", "false").lower() == "true"
        self.approximate = bool(approximate)
        kv = os.path.join(base_path, "kv.db")
        partitions = 0
        while os.path.exists(f"{kv}.{partitions}"):
            partitions += 1
        if not partitions and not self.approximate:
            raise FileNotFoundError(f"{kv}.0")
        self.partitions = partitions
        self._own_ctx = ctx is None  # a borrowed context is used and not closed
        self.ctx = Context(device) if ctx is None else ctx
        self.mph = self.db = None
        try:
            self.mph = self.ctx.mph_load(os.path.join(base_path, "hash.dump"))
            index = os.path.join(base_path, "index_a.db" if self.approximate else "index.db")
            self.db = Database(self.mph, kv, partitions, index, self.approximate, 0 if compact else 1, block_size)
        except Exception:
            self.close()
            raise

    def get_batch(self, blob, offsets) -> dict:
        """Keys blob[offsets[i]:offsets[i+1]]: the dict of Database.get_var
        (status, voff, values, report)."""
        return self.db.get_var(blob, offsets)

    def get(self, key: bytes) -> Optional[bytes]:
        """SyncReader.getAsBytes: the value, or None."""
        r = self.get_batch(np.frombuffer(bytes(key), np.uint8), np.array([0, len(key)], np.uint64))
        return r["values"].tobytes() if r["status"][0] == GET_FOUND else None

    def items(self, batch: int = 1 << 20, first: int = 0, count: Optional[int] = None):
        """The database's (key, value) pairs as bytes, in slot order, `batch`
        slots a call of Database.items; a slot whose address names no record
        is skipped."""
        end = self.db.info()["n"] if count is None else first + count
        for r0 in range(first, end, max(1, batch)):
            r = self.db.items(r0, min(batch, end - r0))
            keys, values = r["keys"].tobytes(), r["values"].tobytes()
            koff, voff = r["koff"].tolist(), r["voff"].tolist()
            for i, st in enumerate(r["status"].tolist()):
                if st == SCAN_OK:
                    yield keys[koff[i]: koff[i + 1]], values[voff[i]: voff[i + 1]]

    def dump_text(self, path, separator=" ", first: int = 0, count: Optional[int] = None, append: bool = False) -> dict:
        """Database.dump_text: the ``key<sep>value`` lines of the slots to `path`; returns the report."""
        return self.db.dump_text(path, separator, first, count, append)

    def diff(self, other: "BSDBReader", upsert=None, removed=None, separator=" ") -> dict:
        """Database.diff: this database against `other`'s (a reader on the same context: ``ctx=self.ctx``)."""
        return self.db.diff(other.db, upsert, removed, separator)

    def close(self):
        for o in (self.db, self.mph, self.ctx if self._own_ctx else None):
            if o is not None:
                o.close()
        self.db = self.mph = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def main(argv=None) -> int:
    import argparse
    ap = argparse.ArgumentParser(prog="python -m bsdb_amd.reader", description="dump a database directory as key<sep>value lines")
    ap.add_argument("--dump", required=True, metavar="OUT", help="the text file to write")
    ap.add_argument("-d", "--db", required=True, help="the database directory")
    ap.add_argument("-s", "--separator", default=" ", help="the one-byte field separator (default: a space)")
    ap.add_argument("--first", type=int, default=0, help="the first slot (default 0)")
    ap.add_argument("--count", type=int, default=None, help="slots to dump (default: to the last)")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    with BSDBReader(a.db, approximate=False, device=a.device) as rd:
        rep = rd.dump_text(a.dump, a.separator, a.first, a.count)
    first_bad = "none" if rep["first_bad"] == SCAN_NONE else rep["first_bad"]
    print(f"slots {rep['slots']}  ok {rep['ok']}  bad_addr {rep['bad_addr']}  not_text {rep['not_text']}  "
          f"text_bytes {rep['text_bytes']}  first_bad {first_bad}")
    return 0 if rep["ok"] == rep["slots"] else 2


if __name__ == "__main__":
    raise SystemExit(main())

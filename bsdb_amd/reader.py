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
"""
from __future__ import annotations

import os
from typing import Optional

import numpy as np

from .native import GET_FOUND, Context, Database


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
    def __init__(self, base_path: str, approximate: Optional[bool] = None, device: int = 0):
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
        self.ctx = Context(device)
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

    def close(self):
        for o in (self.db, self.mph, self.ctx):
            if o is not None:
                o.close()
        self.db = self.mph = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

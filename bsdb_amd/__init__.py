"""bsdb_amd -- MI355X-native index-build hot path for yc-huang/bsdb.

The package holds only what the path needs:
  csrc/           hand-written gfx950 HIP kernels + the C ABI (include/bsdb_mi355x.h)
  native.py       ctypes binding of that C ABI (the product path; no CPU fallback)
  distributed.py  key shards, the histogram collective, the multi-GPU full build
  writer.py       host-side mirror of the reference's BSDBWriter build stages
  reader.py       host-side mirror of the reference's SyncReader over the batched get
  builder.py      the reference's Builder for text input: lines of key<sep>value -> database (build_text, CLI)
  diff.py         two database directories compared on the device: counts and the delta as text (diff_dirs, CLI)
"""
from .native import BsdbError, Context, Database, IndexWriter, Mph, Multi, lib, num_buckets  # noqa: F401
from .reader import BSDBReader  # noqa: F401

__all__ = ["BSDBReader", "BsdbError", "Context", "Database", "IndexWriter", "Mph", "Multi", "lib", "num_buckets"]

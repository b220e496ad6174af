"""Database directories moved beyond 32 bits, for tests/test_high_cases_cpu.py and
tests/test_high_offsets_gpu.py.  Not a test module: pure functions over numpy
and the file system, no device and no subprocess.

A database's records can be put at any file offset without building a large
database: `relocate` copies a directory so that partition p's file is a hole
of shifts[p] bytes followed by the original bytes, and adds the shift to every
address of index.db.  The hole is never written (ftruncate to the final size,
then one pwrite of the original bytes), so a file of 4 GiB costs what its
records cost; it reads as zeros.  Every record keeps its key, its value and its
slot: hash.dump and the config are copied unchanged.

  compact   the address is partition << 56 | file offset: the offset grows by
            shifts[p] (any number of bytes)
  blocked   the address is partition << 56 | pages << 48 | page number << 16 |
            offset in the block: the page number grows by shifts[p] / 4096, so
            the shift is a multiple of 4096

The image an open lays out (get_layout: locate_cases.layout) puts partition 0
at image position 0, so `straddle_shift` places one chosen byte of one chosen
record of partition 0 at image position 2^32."""
import os
import shutil

import numpy as np

PAGE = 4096
FILE_MASK = (1 << 56) - 1
HIGH = 1 << 32


def straddle_shift(offset, x):
    """The shift of partition 0 that puts byte `x` of the record at file `offset` at image position 2^32."""
    shift = HIGH - offset - x
    assert shift >= 0
    return shift


def relocate(src_dir, dst_dir, partitions, fmt, block, shifts):
    """Copies the database of `src_dir` (fmt 0 compact, 1 blocked in blocks of `block` bytes) to `dst_dir` with
    partition p's records shifts[p] bytes further into kv.db.<p>.  Returns the new files' sizes."""
    shifts = [int(s) for s in shifts]
    assert len(shifts) == partitions and all(s >= 0 for s in shifts)
    assert fmt in (0, 1) and (fmt == 0 or (block % PAGE == 0 and all(s % PAGE == 0 for s in shifts)))
    os.makedirs(dst_dir, exist_ok=True)
    sizes = []
    for p in range(partitions):
        with open(os.path.join(src_dir, f"kv.db.{p}"), "rb") as f:
            data = f.read()
        sizes.append(shifts[p] + len(data))
        assert sizes[p] <= (1 << 56 if fmt == 0 else 1 << 44)
        fd = os.open(os.path.join(dst_dir, f"kv.db.{p}"), os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
        try:
            os.ftruncate(fd, sizes[p])
            done = 0
            while done < len(data):
                done += os.pwrite(fd, data[done:], shifts[p] + done)
        finally:
            os.close(fd)
    index = np.fromfile(os.path.join(src_dir, "index.db"), ">u8").astype(np.uint64)
    part = (index >> np.uint64(56)).astype(np.int64)
    assert index.size == 0 or part.max() < partitions                # bit 63 clear, a partition there is
    add = np.array([s if fmt == 0 else (s // PAGE) << 16 for s in shifts], np.uint64)
    if fmt == 0:
        assert all(int(w & np.uint64(FILE_MASK)) + shifts[p] <= FILE_MASK for w, p in zip(index, part))
    else:
        assert all(((int(w) >> 16) & 0xFFFFFFFF) + shifts[p] // PAGE <= 0xFFFFFFFF for w, p in zip(index, part))
    (index + add[part]).astype(">u8").tofile(os.path.join(dst_dir, "index.db"))
    for name in os.listdir(src_dir):
        if name != "index.db" and not name.startswith("kv.db."):
            shutil.copyfile(os.path.join(src_dir, name), os.path.join(dst_dir, name))
    return sizes

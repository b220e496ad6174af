#!/usr/bin/env python3
"""Rate of the record pack of a resident database on the C2 shape; writes one
JSON file (default profiles/merge/c2.json) and prints it.

The database is tools/get_rate.py's: --records records (default 1e8) of
13-byte keys (the device key generator's) with values of 8..64 bytes, compact
layout, 8 partitions, exact mode, indexed by bsdb_kv_build_index and made
resident by bsdb_db_open.  On that one database, in one process, on the same
window of --window slots (default 1e7), each figure the median of --reps timed
steps after --warmup untimed ones (device events; all the values are recorded):
  pack kernel   k_rec_pack<true> alone (bsdb_set_profiling kind 6) within
                bsdb_dev_db_pack of the window into a compact image of 8
                runs, in output bytes per second, against
  text kernel   k_dump_text alone over the same window (kind 4), in output
                bytes per second: the yardstick.  Both copy two sources per
                record through the same piece loop; the pack writes a 3-byte
                header where the dump writes two separator bytes and tests
                every byte.  The bar: the pack's rate is at least half the
                dump's.
  blocked pack  k_rec_pack_blocked alone (kind 6, block size 4096): a figure
  pack call     bsdb_dev_db_pack as a whole (sizes, scans, one wait, the image,
                the key blob, the addresses): a figure
A measurement needs the GPU: without one this fails, it does not fall back.
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from get_rate import PARTS, lib_sha256, median, write_partitions  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=100_000_000)
    ap.add_argument("--window", type=int, default=10_000_000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tmp", default=None, help="directory for the database files (default: a temporary one)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge", "c2.json"))
    a = ap.parse_args()
    import torch
    from bsdb_amd.native import Context
    if not torch.cuda.is_available():
        raise SystemExit("tools/merge_rate.py measures on the GPU; no device is visible")
    n, w = a.records, min(a.window, a.records)
    d = tempfile.mkdtemp(prefix="merge_rate_", dir=a.tmp)
    try:
        with Context(0) as ctx:
            t0 = time.time()
            keys = ctx.gen_keys13(0, n).cpu().numpy().reshape(n, 13)
            kv, ip = os.path.join(d, "kv.db"), os.path.join(d, "index.db")
            write_partitions(kv, keys, 1)
            del keys
            t_files = time.time() - t0
            mph = ctx.kv_build_index(kv, PARTS, 4, ip, None, False)
            db = mph.open_db(kv, PARTS, ip)
            info = db.info()

            def timed(fn):
                ms = []
                for i in range(a.warmup + a.reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn(i)
                    e1.record()
                    e1.synchronize()
                    ms.append(e0.elapsed_time(e1))
                return ms[a.warmup:]

            def kernel_of(kind, call):
                """(the kernel's ms per timed step, the call's)."""
                kernel = []

                def step(i):
                    ctx.set_profiling(True)
                    call()
                    ms, launches, _ = ctx.profile_read(kind)
                    ctx.set_profiling(False)
                    assert launches == 1
                    kernel.append(ms)

                whole = timed(step)
                return kernel[a.warmup:], whole

            ksrc, klen, vsrc, vlen, status, rep = ctx.db_records(db, 0, w)
            assert rep.cpu().tolist()[:3] == [w, w, 0]
            record_bytes = 3 * w + int(klen.sum(dtype=torch.int64)) + int(vlen.sum(dtype=torch.int64))
            # the yardstick: the dump's text kernel over the window
            llen, loff = ctx.db_dump_lengths(db, klen, vlen, status)
            text_bytes = int(loff[w])
            text = torch.empty(text_bytes, dtype=torch.uint8, device="cuda")
            rep0 = ctx.scan_report("cuda")
            dump_kernel, _ = kernel_of(ctx.DUMP_TEXT, lambda: ctx.db_dump_text(
                db, ksrc, klen, vsrc, vlen, status, " ", 0, text=text, llen=llen, loff=loff, text_bytes=text_bytes, report=rep0))
            del text
            # the pack of the same window: compact, then blocked
            out = {}
            for name, bs in (("pack", None), ("pack_blocked", 4096)):
                cap = (2 * record_bytes + PARTS * bs if bs else record_bytes) + 16
                image = torch.empty(cap, dtype=torch.uint8, device="cuda")
                blob = torch.empty(13 * w + 16, dtype=torch.uint8, device="cuda")
                addr = torch.empty(w, dtype=torch.int64, device="cuda")
                off = torch.empty(w + 1, dtype=torch.int64, device="cuda")
                res = {}

                def call():
                    res.update(ctx.db_pack(db, ksrc, klen, vsrc, vlen, PARTS, [0] * PARTS, image=image, blob=blob, addr=addr, off=off,
                                           block_size=bs))

                kernel, whole = kernel_of(ctx.REC_PACK, call)
                image_bytes = sum(res["run_bytes"])
                assert res["blob"].numel() == 13 * w and (image_bytes == record_bytes if bs is None else image_bytes >= record_bytes)
                if bs is None:  # the image is the window's records: checked on its first record
                    k0, v0 = int(klen[0]), int(vlen[0])
                    head = image[:3].cpu().tolist()
                    assert head == [k0, v0 >> 8, v0 & 255]
                out[name] = dict(kernel_ms=median(kernel), kernel_ms_all=kernel, call_ms=median(whole), call_ms_all=whole,
                                 image_bytes=image_bytes, bytes_per_s=image_bytes / (median(kernel) * 1e-3))
                del image, blob, addr, off
            db.close()
            mph.close()
        t_dump = median(dump_kernel)
        dump_rate = text_bytes / (t_dump * 1e-3)
        res = {
            "tool": "merge_rate", "command": f"python tools/merge_rate.py --records {n} --window {w} --warmup {a.warmup} --reps {a.reps}",
            "records": n, "window": w, "partitions": PARTS, "key_len": 13, "value_len": "8..64", "layout": "compact", "mode": "exact",
            "image_bytes": info["image_bytes"], "record_bytes": record_bytes, "text_bytes": text_bytes, "warmup": a.warmup, "reps": a.reps,
            "dump_text_kernel_ms": t_dump, "dump_text_kernel_ms_all": dump_kernel, "dump_text_bytes_per_s": dump_rate,
            "pack_kernel_ms": out["pack"]["kernel_ms"], "pack_kernel_ms_all": out["pack"]["kernel_ms_all"],
            "pack_bytes_per_s": out["pack"]["bytes_per_s"], "pack_over_dump_rate": out["pack"]["bytes_per_s"] / dump_rate,
            "bar_pack_at_least_half_dump": bool(out["pack"]["bytes_per_s"] >= dump_rate / 2),
            "pack_call_ms": out["pack"]["call_ms"], "pack_call_ms_all": out["pack"]["call_ms_all"],
            "pack_blocked_kernel_ms": out["pack_blocked"]["kernel_ms"], "pack_blocked_kernel_ms_all": out["pack_blocked"]["kernel_ms_all"],
            "pack_blocked_image_bytes": out["pack_blocked"]["image_bytes"], "pack_blocked_bytes_per_s": out["pack_blocked"]["bytes_per_s"],
            "pack_blocked_call_ms": out["pack_blocked"]["call_ms"], "pack_blocked_call_ms_all": out["pack_blocked"]["call_ms_all"],
            "setup_s": {"files": t_files}, "library_sha256": lib_sha256()}
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print(json.dumps(res))
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()

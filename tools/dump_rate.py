#!/usr/bin/env python3
"""Rate of the enumeration of a resident database by slot on the C2 shape;
writes one JSON file (default profiles/dump/c2.json) and prints it.

The database is tools/get_rate.py's: --records records (default 1e8) of
13-byte keys (the device key generator's) with values of 8..64 bytes, compact
layout, 8 partitions, exact mode, indexed by bsdb_kv_build_index and made
resident by bsdb_db_open.  On that one database, in one session, each figure
the median of --reps timed steps after --warmup untimed ones (device events;
all the values are recorded):
  records kernel   bsdb_dev_db_records over a window of --window slots (default
                   1e7; step i takes window i of the database), per slot,
                   against
  locate kernel    bsdb_dev_db_locate_fixed over --window random present keys,
                   per query.  The bar: records is at most 1x locate.
  text kernel      k_dump_text alone over the first window (bsdb_set_profiling
                   kind 4), in output bytes per second, against
  gather kernel    bsdb_dev_db_gather over the same window's values.  The
                   bar: the text's rate is at least half the gather's.
  dump_text call   bsdb_dev_db_dump_text (the text kernel and the report)
  host form        bsdb_db_dump_text of the first window to a file in --tmp
                   (host clock; a figure, it has no bar: the copy to the host
                   and the file write bound it)
A measurement needs the GPU: without one this fails, it does not fall back.
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

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
    ap.add_argument("--tmp", default=None, help="directory for the database files and the dump (default: a temporary one)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dump", "c2.json"))
    a = ap.parse_args()
    import torch
    from bsdb_amd.native import GET_WORDS, Context
    if not torch.cuda.is_available():
        raise SystemExit("tools/dump_rate.py measures on the GPU; no device is visible")
    n, w = a.records, min(a.window, a.records)
    windows = max(1, n // w)
    d = tempfile.mkdtemp(prefix="dump_rate_", dir=a.tmp)
    try:
        with Context(0) as ctx:
            t0 = time.time()
            keys = ctx.gen_keys13(0, n).cpu().numpy().reshape(n, 13)
            kv, ip = os.path.join(d, "kv.db"), os.path.join(d, "index.db")
            addr, vlen_np = write_partitions(kv, keys, 1)
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

            # locate and gather, as tools/get_rate.py times them
            idx = np.random.default_rng(2).integers(0, n, w)
            d_keys = torch.from_numpy(np.ascontiguousarray(keys[idx]).reshape(-1)).cuda()
            report = torch.zeros(GET_WORDS, dtype=torch.int64, device="cuda")
            src, vl32, status, _ = ctx.db_locate_fixed(db, d_keys, 13, report=report)
            locate = timed(lambda i: ctx.db_locate_fixed(db, d_keys, 13, src=src, vlen=vl32, status=status, report=report))
            assert not status.any().item()
            del d_keys, src, vl32, status
            # the records kernel, a window a step
            rep0 = ctx.scan_report("cuda")
            records = timed(lambda i: ctx.db_records(db, (i % windows) * w, w, report=rep0))
            ksrc, klen, vsrc, vlen, status, rep = ctx.db_records(db, 0, w)
            assert rep.cpu().tolist()[:3] == [w, w, 0]
            # the window's values gathered; its text
            voff = ctx.edge_offsets(vlen)
            value_bytes = int(voff[w])
            out = torch.empty(value_bytes, dtype=torch.uint8, device="cuda")
            gather = timed(lambda i: ctx.db_gather(db, vsrc, voff, values=out, value_bytes=value_bytes))
            llen, loff = ctx.db_dump_lengths(db, klen, vlen, status)
            text_bytes = int(loff[w])
            assert text_bytes == 15 * w + value_bytes
            text = torch.empty(text_bytes, dtype=torch.uint8, device="cuda")
            kernel = []

            def dump(i):
                ctx.set_profiling(True)
                ctx.db_dump_text(db, ksrc, klen, vsrc, vlen, status, " ", 0, text=text, llen=llen, loff=loff, text_bytes=text_bytes,
                                 report=rep0)
                ms, launches, _ = ctx.profile_read(ctx.DUMP_TEXT)
                ctx.set_profiling(False)
                assert launches == 1
                kernel.append(ms)

            call = timed(dump)
            kernel = kernel[a.warmup:]
            # the text is the window's records: checked on its first and last lines and its line count
            head = text[:200].cpu().numpy().tobytes().split(b"\n")[0]
            k0, v0 = int(klen[0]), int(vlen[0])
            assert len(head) == k0 + 1 + v0 and head[k0: k0 + 1] == b" "
            assert int((text == 0x0A).sum()) >= w and int(text[-1]) == 0x0A
            del out
            # the host form, the first window to a file
            path = os.path.join(d, "dump.txt")
            host = []
            for i in range(a.warmup + a.reps):
                t0 = time.perf_counter()
                hrep = db.dump_text(path, count=w)
                host.append(time.perf_counter() - t0)
            assert hrep["slots"] == w and hrep["text_bytes"] == text_bytes == os.path.getsize(path)
            db.close()
            mph.close()
        t_loc, t_rec, t_gat, t_txt, t_call, t_host = (median(x) for x in (locate, records, gather, kernel, call, host[a.warmup:]))
        gather_rate, text_rate = value_bytes / (t_gat * 1e-3), text_bytes / (t_txt * 1e-3)
        res = {
            "tool": "dump_rate", "records": n, "window": w, "partitions": PARTS, "key_len": 13, "value_len": "8..64",
            "layout": "compact", "mode": "exact", "image_bytes": info["image_bytes"], "value_bytes": value_bytes,
            "text_bytes": text_bytes, "warmup": a.warmup, "reps": a.reps,
            "records_ms": t_rec, "records_ns_per_slot": t_rec * 1e6 / w, "records_ms_all": records,
            "locate_ms": t_loc, "locate_ns_per_query": t_loc * 1e6 / w, "locate_ms_all": locate,
            "records_over_locate": t_rec / t_loc, "bar_records_at_most_1x_locate": bool(t_rec <= t_loc),
            "gather_ms": t_gat, "gather_bytes_per_s": gather_rate, "gather_ms_all": gather,
            "text_kernel_ms": t_txt, "text_bytes_per_s": text_rate, "text_kernel_ms_all": kernel,
            "text_over_gather_rate": text_rate / gather_rate, "bar_text_at_least_half_gather": bool(text_rate >= gather_rate / 2),
            "dump_text_call_ms": t_call, "dump_text_call_ms_all": call,
            "host_form_s": t_host, "host_form_bytes_per_s": text_bytes / t_host, "host_form_s_all": host[a.warmup:],
            "host_form_not_text": hrep["not_text"], "setup_s": {"files": t_files}, "library_sha256": lib_sha256()}
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print(json.dumps(res))
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()

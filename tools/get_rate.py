#!/usr/bin/env python3
"""Rate of the batched get on the C2 shape; prints one JSON line.

The database: --records records (default 1e8) of 13-byte keys (the device key
generator's) with values of 8..64 bytes, compact layout, 8 partitions, exact
mode, written to a temporary directory, indexed by bsdb_kv_build_index and
made resident by bsdb_db_open.  The queries: --queries (default 1e7) uniformly
random present keys per step.  Reported, each the median of --reps timed
steps after --warmup untimed ones:
  host form        bsdb_db_get_fixed from host keys to host values (host clock
                   around the call, which ends in a device synchronise)
  locate kernel    bsdb_dev_db_locate_fixed alone (device events)
  gather kernel    bsdb_dev_db_gather alone (device events), and its output
                   bytes per second
  verify           bsdb_dev_verify_fixed over the SAME keys on the same
                   database (device events): the same chain minus the record
                   read.  The one bar: locate's time per query is at most
                   twice verify's time per record ("locate_over_verify").
A measurement needs the GPU: without one this fails, it does not fall back.
"""
import argparse
import hashlib
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PARTS = 8


def lib_sha256():
    path = os.environ.get("BSDB_LIB") or os.path.join(ROOT, "bsdb_amd", "libbsdb_mi355x.so")
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for b in iter(lambda: f.read(1 << 20), b""):
            h.update(b)
    return h.hexdigest()


def write_partitions(kv, keys, seed):
    """kv.<p> in the compact layout ([kLen][vLen u16 BE][key][value], record i in partition i % PARTS), each
    partition compacted from fixed-stride rows; returns every record's address and value length."""
    n = keys.shape[0]
    addr = np.zeros(n, np.uint64)
    vlen = np.zeros(n, np.uint8)
    rng = np.random.default_rng(seed)
    for p in range(PARTS):
        idx = np.arange(p, n, PARTS)
        m = idx.size
        vl = rng.integers(8, 65, m).astype(np.int64)
        rows = np.empty((m, 16 + 64), np.uint8)
        rows[:, 0] = 13
        rows[:, 1] = 0
        rows[:, 2] = vl
        rows[:, 3:16] = keys[idx]
        rows[:, 16:] = rng.integers(0, 256, (m, 64), dtype=np.uint8)
        size = 16 + vl
        rows[np.arange(80)[None, :] < size[:, None]].tofile(f"{kv}.{p}")
        pos = np.cumsum(size) - size
        addr[idx] = (np.uint64(p) << np.uint64(56)) | pos.astype(np.uint64)
        vlen[idx] = vl
    return addr, vlen


def median(xs):
    return float(np.median(np.asarray(xs, np.float64)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=100_000_000)
    ap.add_argument("--queries", type=int, default=10_000_000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tmp", default=None, help="directory for the database files (default: a temporary one)")
    a = ap.parse_args()
    import torch
    from bsdb_amd.native import GET_WORDS, Context
    if not torch.cuda.is_available():
        raise SystemExit("tools/get_rate.py measures on the GPU; no device is visible")
    n, nq = a.records, a.queries
    d = tempfile.mkdtemp(prefix="get_rate_", dir=a.tmp)
    try:
        with Context(0) as ctx:
            t0 = time.time()
            keys = ctx.gen_keys13(0, n).cpu().numpy().reshape(n, 13)
            kv, ip = os.path.join(d, "kv.db"), os.path.join(d, "index.db")
            addr, vlen = write_partitions(kv, keys, 1)
            t_files = time.time() - t0
            t0 = time.time()
            mph = ctx.kv_build_index(kv, PARTS, 4, ip, None, False)
            t_build = time.time() - t0
            t0 = time.time()
            db = mph.open_db(kv, PARTS, ip)
            t_open = time.time() - t0
            info = db.info()
            idx = np.random.default_rng(2).integers(0, n, nq)
            qkeys = np.ascontiguousarray(keys[idx])
            want_bytes = int(vlen[idx].astype(np.int64).sum())
            # the host form
            host = []
            for i in range(a.warmup + a.reps):
                t0 = time.perf_counter()
                res = db.get_fixed(qkeys, 13, value_cap=want_bytes)
                host.append(time.perf_counter() - t0)
            rep = res["report"]
            assert rep["found"] == nq and rep["value_bytes"] == want_bytes, rep
            # the kernels, on device-resident keys
            d_keys = torch.from_numpy(qkeys.reshape(-1)).cuda()
            d_addr = torch.from_numpy(addr[idx].astype(np.int64)).cuda()
            E, values, sigbits = (torch.from_numpy(x.view(np.int64)).cuda() for x in mph.export())
            index = torch.from_numpy(np.fromfile(ip, np.int64)).cuda()
            report = torch.zeros(GET_WORDS, dtype=torch.int64, device="cuda")
            src, vl32, status, _ = ctx.db_locate_fixed(db, d_keys, 13, report=report)
            voff = ctx.edge_offsets(vl32)
            out = torch.empty(want_bytes, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            assert int(voff[nq]) == want_bytes

            def timed(fn):
                ms = []
                for i in range(a.warmup + a.reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    e1.synchronize()
                    ms.append(e0.elapsed_time(e1))
                return ms[a.warmup:]

            locate = timed(lambda: ctx.db_locate_fixed(db, d_keys, 13, src=src, vlen=vl32, status=status, report=report))
            gather = timed(lambda: ctx.db_gather(db, src, voff, values=out, value_bytes=want_bytes))
            counters = []
            verify = timed(lambda: counters.append(ctx.verify_fixed(d_keys, 13, n, E, values, index, width=4,
                                                                    sigbits=sigbits, addr=d_addr)))
            assert counters[-1][:5] == (nq, 0, nq, 0, 0), counters[-1]
            # the gathered bytes are the host form's
            assert np.array_equal(out.cpu().numpy(), res["values"])
            db.close()
            mph.close()
        t_locate, t_gather, t_verify, t_host = median(locate), median(gather), median(verify), median(host[a.warmup:])
        print(json.dumps({
            "tool": "get_rate", "records": n, "queries": nq, "partitions": PARTS, "key_len": 13, "value_len": "8..64",
            "layout": "compact", "mode": "exact", "image_bytes": info["image_bytes"], "value_bytes": want_bytes,
            "warmup": a.warmup, "reps": a.reps,
            "host_form_s": t_host, "host_form_queries_per_s": nq / t_host,
            "locate_ms": t_locate, "locate_ns_per_query": t_locate * 1e6 / nq, "locate_queries_per_s": nq / (t_locate * 1e-3),
            "locate_ms_all": locate,
            "gather_ms": t_gather, "gather_bytes_per_s": want_bytes / (t_gather * 1e-3), "gather_ms_all": gather,
            "verify_ms": t_verify, "verify_ns_per_record": t_verify * 1e6 / nq, "verify_ms_all": verify,
            "locate_over_verify": t_locate / t_verify, "bar_locate_at_most_2x_verify": bool(t_locate <= 2 * t_verify),
            "setup_s": {"files": t_files, "build": t_build, "open": t_open},
            "library_sha256": lib_sha256()}))
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Measures the value compare of the diff of two resident databases
(bsdb_dev_db_diff, k_diff_values) on the C2 shape of tools/text_rate.py: lines
of a 13-byte key, a space and a value of 8..64 bytes.  Database A is the text
built compact in 8 partitions, database B the same text built blocked in 2:
every record is SAME, so every value byte is compared, and B's values lie
where another layout put them.  Writes one JSON file (default
profiles/diff/c2.json) with the library's sha256.  Medians of 5 timed runs
after 2 warm-ups, all values kept.

  diff_values    k_diff_values alone per window of A's slots (the library's own
                 event pair around the launch, bsdb_set_profiling kind 5), on
                 located records: records -> key gather -> locate in B are done
                 once per window, outside the timed part
  check_values   in the same process, on the same records: k_check_values alone
                 (kind 3) per chunk of the text against database A, as
                 tools/check_rate.py measures it
The yardstick is check_values in GB/s of compared bytes: both kernels read two
sources and write nothing; the check's second source is the text, sequential,
the diff's is B's image, scattered.  With --once every leg runs once and
nothing is written: the form to put under a kernel trace.  A measurement needs
the GPU: without one this fails.
"""
import argparse
import hashlib
import json
import os
import shutil
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from text_rate import CHUNK, RUNS, WARM, make_text, timed  # noqa: E402

WINDOW = 1 << 22  # slots of one bsdb_dev_db_diff call: the default chunk of bsdb_db_diff


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lines", type=int, default=10_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diff", "c2.json"))
    ap.add_argument("--once", action="store_true", help="every leg once, nothing written")
    ap.add_argument("--tmp", default=None, help="directory for the text and the databases (default: a temporary one)")
    a = ap.parse_args()
    import torch
    from bsdb_amd import Context
    from bsdb_amd.native import DIFF_FIELDS, DIFF_NONE, LIB_PATH
    if not torch.cuda.is_available():
        raise SystemExit("tools/diff_rate.py measures on the GPU; no device is visible")

    tmp = a.tmp or tempfile.mkdtemp(prefix="diff_rate_")
    os.makedirs(tmp, exist_ok=True)
    text = make_text(a.lines)
    path = os.path.join(tmp, "c2.txt")
    text.tofile(path)
    res = {"shape": "C2: 13-byte key, space, 8..64-byte value, \\n", "lines": a.lines, "text_bytes": int(text.size),
           "A": "compact, 8 partitions", "B": "blocked (4096), 2 partitions", "window_slots": WINDOW, "warmups": WARM, "runs": RUNS,
           "command": "python tools/diff_rate.py --lines %d" % a.lines,
           "library_sha256": hashlib.sha256(open(LIB_PATH, "rb").read()).hexdigest()}
    measure = (lambda fn: fn()) if a.once else timed

    with Context(0) as ctx:
        def build(name, parts, fmt):
            d = os.path.join(tmp, name)
            os.makedirs(d, exist_ok=True)
            kv, ix, ia = (os.path.join(d, f) for f in ("kv.db", "index.db", "index_a.db"))
            mph, rep = ctx.text_build([path], " ", kv, parts, 4, ix, ia, fmt=fmt, block_size=4096)
            assert rep["records"] == a.lines, rep
            return mph, mph.open_db(kv, parts, ix, fmt=fmt, block_size=4096)

        mph_a, db_a = build("A", 8, 0)
        mph_b, db_b = build("B", 2, 1)

        def profiled(kind, call):
            ctx.set_profiling(True)
            call()
            torch.cuda.synchronize()
            ms, launches, _ = ctx.profile_read(kind)
            ctx.profile_read(ctx.SCAN)
            ctx.set_profiling(False)
            assert launches == 1
            return ms / 1e3

        # ---- the diff: windows of A's slots against B
        windows = []
        for first in range(0, a.lines, WINDOW):
            count = min(WINDOW, a.lines - first)
            ksrc, klen, vsrc, vlen, st_a, _ = ctx.db_records(db_a, first, count)
            koff = ctx.edge_offsets(klen)
            src, vl, located, _ = ctx.db_locate_var(db_b, ctx.db_gather(db_a, ksrc, koff), koff)
            status, rep = ctx.db_diff(db_a, db_b, vsrc, vlen, st_a, src, vl, located.clone(), slot_base=first)
            rep = dict(zip(DIFF_FIELDS, rep.cpu().numpy().view(np.uint64).tolist()))
            assert rep["same"] == rep["slots"] == count and rep["first_diff"] == DIFF_NONE, rep

            def diff_values():
                st = located.clone()
                return profiled(ctx.DIFF_VALUES, lambda: ctx.db_diff(db_a, db_b, vsrc, vlen, st_a, src, vl, st, slot_base=first))

            dv = measure(diff_values)
            if not a.once:
                windows.append({"first": first, "slots": count, "compared_bytes": rep["compared_bytes"], "diff_values_s": dv,
                                "diff_values_GBps_compared": rep["compared_bytes"] / dv["median"] / 1e9})
            del ksrc, klen, vsrc, vlen, st_a, koff, src, vl, located, status

        # ---- the check, on the same records: chunks of the text against A (tools/check_rate.py's check_values leg)
        cuts, lo = [], 0
        while lo < text.size:
            hi = min(text.size, lo + CHUNK)
            if hi < text.size:
                hi = lo + int(np.flatnonzero(text[lo:hi] == 10)[-1]) + 1
            cuts.append((lo, hi))
            lo = hi
        chunks = []
        for lo, hi in cuts:
            n = hi - lo
            t = torch.empty(n + 16, dtype=torch.uint8, device="cuda")
            t[:n] = torch.from_numpy(text[lo:hi]).cuda()
            desc = torch.empty((4, n // 4 + 1), dtype=torch.int32, device="cuda")
            blob = torch.empty(n + 16, dtype=torch.uint8, device="cuda")
            _, rep = ctx.text_split(t, " ", nbytes=n, desc=desc)
            k = int(rep[1])
            out = ctx.text_pack(t, desc, k, 1, [0], nbytes=n, blob=blob, want_image=False)
            src, dbvlen, located, _ = ctx.db_locate_var(db_a, out["blob"], out["off"])
            total = int(dbvlen.sum())

            def check_values():
                st = located.clone()
                return profiled(ctx.CHECK_VALUES, lambda: ctx.db_check(db_a, t, desc[2], desc[3], src, dbvlen, st, nbytes=n, count=k))

            cv = measure(check_values)
            if not a.once:
                chunks.append({"bytes": n, "records": k, "compared_bytes": total, "check_values_s": cv,
                               "check_values_GBps_compared": total / cv["median"] / 1e9})
            del t, desc, blob, out, src, dbvlen, located
        for o in (db_a, db_b, mph_a, mph_b):
            o.close()
    if not a.tmp:
        shutil.rmtree(tmp, ignore_errors=True)
    if a.once:
        return

    def spread(rows, key):
        # the run's own repetition spread: (max - min) / median of the per-run totals
        runs = [sum(r[key]["values"][i] for r in rows) for i in range(RUNS)]
        return (max(runs) - min(runs)) / float(np.median(runs))

    d_bytes, c_bytes = sum(w["compared_bytes"] for w in windows), sum(c["compared_bytes"] for c in chunks)
    d_s, c_s = sum(w["diff_values_s"]["median"] for w in windows), sum(c["check_values_s"]["median"] for c in chunks)
    assert d_bytes == c_bytes, (d_bytes, c_bytes)
    res["diff"] = {"windows": windows, "diff_values_total_s": d_s, "compared_bytes": d_bytes,
                   "diff_values_GBps_compared": d_bytes / d_s / 1e9, "repetition_spread": spread(windows, "diff_values_s")}
    res["check"] = {"chunks": chunks, "check_values_total_s": c_s, "compared_bytes": c_bytes,
                    "check_values_GBps_compared": c_bytes / c_s / 1e9, "repetition_spread": spread(chunks, "check_values_s")}
    res["diff_values_over_check_values"] = d_s / c_s
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"lines": a.lines, "compared_bytes": d_bytes, "diff_values_GBps_compared": res["diff"]["diff_values_GBps_compared"],
                      "check_values_GBps_compared": res["check"]["check_values_GBps_compared"],
                      "diff_values_over_check_values": res["diff_values_over_check_values"],
                      "diff_spread": res["diff"]["repetition_spread"], "check_spread": res["check"]["repetition_spread"]}))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Measures the check of a database against text input (bsdb_db_check_text,
bsdb_dev_db_check and its kernels) on the C2 shape of tools/text_rate.py: lines
of a 13-byte key, a space and a value of 8..64 bytes, ended by "\\n"; compact
layout, 8 partitions.  Writes one JSON file (default profiles/check/c2.json)
with the library's sha256.  Medians of 5 timed runs after 2 warm-ups, all
values kept.

Per chunk of the text (the chunks bsdb_db_check_text would make), device events
around
  check_values    k_check_values alone (the library's own event pair around the
                  launch, bsdb_set_profiling kind 3)
  check           the whole per-chunk check: split + key blob + locate + check
  gather          in the same run, on the same located values, the unchanged
                  k_get_gather (bsdb_dev_db_gather)
  split_pack      and split + compact pack (image and blob), as bsdb_text_build
                  runs them
The yardstick is the gather: k_check_values does the gather's search once and
its bounded reads twice and has no store, so it is expected at no more than
2 x k_get_gather over the same values ("check_values_over_gather").  For
context only: the wall clock of bsdb_db_check_text beside bsdb_text_build's.
With --once every leg runs once and nothing is written: the form to put under a
kernel trace.  A measurement needs the GPU: without one this fails.
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lines", type=int, default=10_000_000)
    ap.add_argument("--partitions", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "check", "c2.json"))
    ap.add_argument("--once", action="store_true", help="every leg once, nothing written")
    ap.add_argument("--tmp", default=None, help="directory for the text and the database (default: a temporary one)")
    a = ap.parse_args()
    import torch
    from bsdb_amd import Context
    from bsdb_amd.native import CHECK_FIELDS, CHECK_NONE, LIB_PATH
    if not torch.cuda.is_available():
        raise SystemExit("tools/check_rate.py measures on the GPU; no device is visible")

    tmp = a.tmp or tempfile.mkdtemp(prefix="check_rate_")
    os.makedirs(tmp, exist_ok=True)
    text = make_text(a.lines)
    path = os.path.join(tmp, "c2.txt")
    text.tofile(path)
    res = {"shape": "C2: 13-byte key, space, 8..64-byte value, \\n", "lines": a.lines, "text_bytes": int(text.size),
           "partitions": a.partitions, "warmups": WARM, "runs": RUNS,
           "library_sha256": hashlib.sha256(open(LIB_PATH, "rb").read()).hexdigest()}
    cuts, lo = [], 0
    while lo < text.size:
        hi = min(text.size, lo + CHUNK)
        if hi < text.size:
            hi = lo + int(np.flatnonzero(text[lo:hi] == 10)[-1]) + 1
        cuts.append((lo, hi))
        lo = hi
    measure = (lambda fn: fn()) if a.once else timed

    def ev_s(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        return s.elapsed_time(e) / 1e3

    with Context(0) as ctx:
        db_dir = os.path.join(tmp, "db")
        os.makedirs(db_dir, exist_ok=True)
        kv, ix, ia = (os.path.join(db_dir, f) for f in ("kv.db", "index.db", "index_a.db"))

        def text_build():
            mph, rep = ctx.text_build([path], " ", kv, a.partitions, 4, ix, ia)
            assert rep["records"] == a.lines, rep
            return mph

        mph = text_build()
        db = mph.open_db(kv, a.partitions, ix)
        chunks = []
        for lo, hi in cuts:
            n = hi - lo
            t = torch.empty(n + 16, dtype=torch.uint8, device="cuda")
            t[:n] = torch.from_numpy(text[lo:hi]).cuda()
            desc = torch.empty((4, n // 4 + 1), dtype=torch.int32, device="cuda")
            image = torch.empty(n + n // 2 + 16, dtype=torch.uint8, device="cuda")
            blob = torch.empty(n + 16, dtype=torch.uint8, device="cuda")
            state = {}

            def split_pack():
                _, rep = ctx.text_split(t, " ", nbytes=n, desc=desc)
                ctx.text_pack(t, desc, int(rep[1]), a.partitions, [0] * a.partitions, nbytes=n, image=image, blob=blob)

            def check():
                _, rep = ctx.text_split(t, " ", nbytes=n, desc=desc)
                k = int(rep[1])
                out = ctx.text_pack(t, desc, k, 1, [0], nbytes=n, blob=blob, want_image=False)
                src, dbvlen, status, _ = ctx.db_locate_var(db, out["blob"], out["off"])
                state.update(k=k, src=src, dbvlen=dbvlen)
                state["status"], state["report"] = ctx.db_check(db, t, desc[2], desc[3], src, dbvlen, status, nbytes=n, count=k)

            def check_values():
                # the check on located values, the library's own events around k_check_values read back
                ctx.set_profiling(True)
                status = torch.zeros(state["k"], dtype=torch.uint8, device="cuda")
                ctx.db_check(db, t, desc[2], desc[3], state["src"], state["dbvlen"], status, nbytes=n, count=state["k"])
                torch.cuda.synchronize()
                ms, launches, _ = ctx.profile_read(ctx.CHECK_VALUES)
                ctx.profile_read(ctx.SCAN)
                ctx.set_profiling(False)
                assert launches == 1
                return ms / 1e3

            ck = measure(lambda: ev_s(check))
            k = state["k"]
            rep = dict(zip(CHECK_FIELDS, state["report"].cpu().numpy().view(np.uint64).tolist()))
            assert rep["ok"] == rep["records"] == k and rep["first_bad"] == CHECK_NONE, rep
            cv = measure(check_values)
            voff = ctx.edge_offsets(state["dbvlen"])
            total = int(voff[k])
            out = torch.empty(total, dtype=torch.uint8, device="cuda")
            ga = measure(lambda: ev_s(lambda: ctx.db_gather(db, state["src"], voff, values=out, value_bytes=total)))
            sp = measure(lambda: ev_s(split_pack))
            if not a.once:
                chunks.append({"bytes": n, "records": k, "value_bytes": total, "check_values_s": cv, "check_s": ck, "gather_s": ga,
                               "split_pack_s": sp, "check_values_over_gather": cv["median"] / ga["median"],
                               "check_over_split_pack": ck["median"] / sp["median"],
                               "check_values_GBps_compared": total / cv["median"] / 1e9})
            del t, desc, image, blob, out, voff, state
        if not a.once:
            tot = {k: sum(c[k]["median"] for c in chunks) for k in ("check_values_s", "check_s", "gather_s", "split_pack_s")}
            res["kernels"] = {"chunks": chunks, **{k.replace("_s", "_total_s"): v for k, v in tot.items()},
                              "check_values_over_gather": tot["check_values_s"] / tot["gather_s"],
                              "bar_check_values_at_most_2x_gather": bool(tot["check_values_s"] <= 2 * tot["gather_s"])}
            # for context: the host forms end to end
            last = {}

            def host_check():
                last.update(db.check_text([path]))

            hc = timed(host_check)
            assert last["ok"] and last["check"]["ok"] == a.lines, last
            db.close()
            mph.close()
            tb = timed(lambda: text_build().close())
            res["end_to_end"] = {"check_text_s": hc, "text_build_s": tb, "check_Mrecords_per_s": a.lines / hc["median"] / 1e6}
        else:
            db.close()
            mph.close()
    if not a.tmp:
        shutil.rmtree(tmp, ignore_errors=True)
    if a.once:
        return
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"lines": a.lines, "text_bytes": res["text_bytes"],
                      **{k: res["kernels"][k] for k in ("check_values_total_s", "gather_total_s", "check_total_s",
                                                        "split_pack_total_s", "check_values_over_gather",
                                                        "bar_check_values_at_most_2x_gather")},
                      "check_text_s": hc["median"], "text_build_s": tb["median"]}))


if __name__ == "__main__":
    main()

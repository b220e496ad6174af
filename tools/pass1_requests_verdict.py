"""Verdicts of the pass-1 request A/B and of the pass-2 span A/B (DESIGN §4.1,
profiles/pass1_requests/, profiles/pass2_span/).

Reads DIR/<name>.jsonl (bench.py result lines of alternated runs, one file
per library: parent, req_a, req_b, req_c or span_a, span_ab, span_c, all,
final) and prints, per library, the
median / min / max of ms_per_step and of each pass's kernel time, and whether
its median gain over the parent exceeds the parent's own max - min spread
(the bar a change has to clear to stay in the default kernel).
usage: python tools/pass1_requests_verdict.py DIR [OUT_JSON]"""
import json
import os
import statistics
import sys


def column(path, get):
    return [get(json.loads(line)) for line in open(path) if line.strip()]


def main():
    d = sys.argv[1]
    fields = {"ms_per_step": lambda r: r["ms_per_step"], "pass1_ms": lambda r: r["kernel_ms_per_step"]["pass1"],
              "pass2_ms": lambda r: r["kernel_ms_per_step"]["pass2"]}
    out = {}
    # profiles/pass1_requests/: req_a, req_b, req_c; profiles/pass2_span/: span_a, span_ab, span_c, final
    # profiles/launch_length/: final (the default launch length), chunk_2p<k> (bench.py --chunk 2^k)
    # profiles/pass1_insert/: ins_slot, ins_map, ins_add64, ins_slot_map, ins_slot_cur_map, all, final
    names = ["parent", "req_a", "req_b", "req_c", "span_a", "span_ab", "span_c",
             "ins_slot", "ins_map", "ins_add64", "ins_slot_map", "ins_slot_cur_map", "all", "final"]
    names += sorted(f[:-6] for f in os.listdir(d) if f.startswith("chunk_2p") and f.endswith(".jsonl"))
    for name in names:
        path = os.path.join(d, name + ".jsonl")
        if not os.path.exists(path):
            continue
        out[name] = {}
        for f, get in fields.items():
            v = column(path, get)
            out[name][f] = {"runs": v, "median": statistics.median(v), "min": min(v), "max": max(v)}
    for name, o in out.items():
        for f in fields:
            p = out["parent"][f]
            spread = p["max"] - p["min"]
            gain = p["median"] - o[f]["median"]
            o[f]["gain_vs_parent_median"] = gain
            o[f]["parent_spread"] = spread
            o[f]["clears_spread"] = name != "parent" and gain > spread
    for name, o in out.items():
        print(name, " ".join(f"{f}: median {o[f]['median']:.3f} [{o[f]['min']:.3f}, {o[f]['max']:.3f}] "
                             f"gain {o[f]['gain_vs_parent_median']:+.3f} (spread {o[f]['parent_spread']:.3f}) "
                             f"{'CLEARS' if o[f]['clears_spread'] else '-'}" for f in fields))
    if len(sys.argv) > 2:
        json.dump(out, open(sys.argv[2], "w"), indent=1)


if __name__ == "__main__":
    main()

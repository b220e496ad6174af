"""What changed between two database directories, on the device
(bsdb_db_diff): both are made resident on one context, every slot of A is
looked up in B and every slot of B in A, and the values are compared image
against image.  The delta comes out as ``key<sep>value`` lines that
``BSDBWriter.build_text`` and ``check_text`` read: `upsert` holds B's records
that A does not hold or holds with another value (in B's slot order),
`removed` A's records whose key B does not hold (in A's slot order).

    python -m bsdb_amd.diff A_DIR B_DIR [--upsert F] [--removed F] [-s SEP]

prints one line of counts per direction; exit status 0 when the two hold the
same records, 2 when they do not.  Exact databases only; both must fit the
device together.  Applying a delta: build the two files into small databases
(``build_text``) and merge them over A (``python -m bsdb_amd.merge``).
"""
from __future__ import annotations

from .native import DIFF_NONE, DIFF_STATUS_NAMES
from .reader import BSDBReader


def diff_dirs(a_dir: str, b_dir: str, upsert=None, removed=None, separator=" ", device: int = 0) -> dict:
    """Database.diff of the databases in a_dir (A) and b_dir (B): {"ab", "ba", "upsert", "removed", "identical"}."""
    with BSDBReader(a_dir, approximate=False, device=device) as a:
        with BSDBReader(b_dir, approximate=False, ctx=a.ctx) as b:
            return a.diff(b, upsert, removed, separator)


def _line(name: str, rep: dict) -> str:
    first = "none" if rep["first_diff"] == DIFF_NONE else rep["first_diff"]
    return (f"{name}  slots {rep['slots']}  " + "  ".join(f"{k} {rep[k]}" for k in DIFF_STATUS_NAMES)
            + f"  first_diff {first}  compared_bytes {rep['compared_bytes']}")


def main(argv=None) -> int:
    import argparse
    ap = argparse.ArgumentParser(prog="python -m bsdb_amd.diff", description="compare two database directories on the device")
    ap.add_argument("a_dir", metavar="A_DIR", help="the database the delta starts from")
    ap.add_argument("b_dir", metavar="B_DIR", help="the database the delta leads to")
    ap.add_argument("--upsert", metavar="F", default=None, help="write B's added and changed records here, as key<sep>value lines")
    ap.add_argument("--removed", metavar="F", default=None, help="write A's records that B does not hold here")
    ap.add_argument("-s", "--separator", default=" ", help="the one-byte field separator (default: a space)")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    res = diff_dirs(a.a_dir, a.b_dir, a.upsert, a.removed, a.separator, a.device)
    print(_line("A->B", res["ab"]))
    print(_line("B->A", res["ba"]))
    return 0 if res["identical"] else 2


if __name__ == "__main__":
    raise SystemExit(main())

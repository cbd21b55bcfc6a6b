"""Do two runs launch the same kernels?  The check of a host-only routing change, beside tools/device_asm_hash.py.

    python tools/compare_kernel_trace.py A_kernel_trace.csv B_kernel_trace.csv [--by COLUMN]

A and B are `rocprofv3 --kernel-trace --output-format csv` outputs of the same seeded program in two trees (a fresh process each, the
program after `--`, no counters in that run).  Per stream, the streams taken in the order of their first dispatch, the sequences of
(kernel name, grid, workgroup, LDS bytes) must be equal: prints the first difference and exits 1, or the counts and exits 0.
The stream of a dispatch is its Stream_Id column (Queue_Id where the trace has none; --by names another column, `--by none` compares
the whole trace as one sequence in dispatch order)."""
import argparse
import csv
import sys


def streams(path, by):
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    if not rows:
        sys.exit(f"{path}: no dispatches")
    order = "Dispatch_Id" if "Dispatch_Id" in rows[0] else "Start_Timestamp"
    rows.sort(key=lambda r: int(r[order]))
    col = by or ("Stream_Id" if "Stream_Id" in rows[0] else "Queue_Id")
    out = {}                                               # (a dict keeps the order of first appearance)
    for r in rows:
        launch = (r["Kernel_Name"], tuple(int(r["Grid_Size_" + a]) for a in "XYZ"), tuple(int(r["Workgroup_Size_" + a]) for a in "XYZ"),
                  int(r.get("LDS_Block_Size", 0) or 0))
        out.setdefault("all" if col == "none" else r[col], []).append(launch)
    return list(out.values())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--by")
    args = ap.parse_args()
    A, B = streams(args.a, args.by), streams(args.b, args.by)
    for i, (sa, sb) in enumerate(zip(A, B)):
        for j, (x, y) in enumerate(zip(sa, sb)):
            if x != y:
                print(f"stream {i}, dispatch {j} differs:\n  A: {x}\n  B: {y}")
                sys.exit(1)
        if len(sa) != len(sb):
            longer, name = (sa, "A") if len(sa) > len(sb) else (sb, "B")
            print(f"stream {i}: A has {len(sa)} dispatches, B {len(sb)}; the first one only {name} has:\n  {longer[min(len(sa), len(sb))]}")
            sys.exit(1)
    if len(A) != len(B):
        print(f"A uses {len(A)} streams, B {len(B)}")
        sys.exit(1)
    print(f"same launches: {sum(map(len, A))} dispatches on {len(A)} streams ({', '.join(str(len(s)) for s in A)})")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Two rocprofv3 kernel traces (csv output directories) of tools/batch_trace_workload.py: the same kernels in the same dispatch order with the same grid,
workgroup and LDS sizes?  Per section of the workload: the kernel count and "identical" or the first difference.
    python tools/compare_kernel_traces.py <trace dir A> <trace dir B>"""
import csv, glob, sys


def load(d):
    f = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)
    assert len(f) == 1, f
    rows = list(csv.DictReader(open(f[0])))
    key = "Dispatch_Id" if "Dispatch_Id" in rows[0] else "Start_Timestamp"
    rows.sort(key=lambda r: int(r[key]))
    sig = lambda r: (r["Kernel_Name"], r.get("Grid_Size_X"), r.get("Grid_Size_Y"), r.get("Grid_Size_Z"), r.get("Workgroup_Size_X"), r.get("Workgroup_Size_Y"),
                     r.get("Workgroup_Size_Z"), r.get("LDS_Block_Size"))
    return [sig(r) for r in rows], list(rows[0].keys())


def sections(sigs):
    """split at two exp-table launches back to back"""
    out, cur, i = [], [], 0
    while i < len(sigs):
        if "exp_table" in sigs[i][0] and i + 1 < len(sigs) and "exp_table" in sigs[i + 1][0]:
            out.append(cur); cur = []; i += 2
        else:
            cur.append(sigs[i]); i += 1
    out.append(cur)
    return out


a, cols = load(sys.argv[1])
b, _ = load(sys.argv[2])
print("columns:", cols)
print("kernels:", len(a), len(b))
sa, sb = sections(a), sections(b)
names = ["setup", "batch_copy_n3", "batch_copy_n17", "batch_copy_n33", "batch_nocopy_n3", "speculative", "append_many", "pipeline_two_stage", "pipeline_single_gate_up_cut", "end"]
print("sections:", len(sa), len(sb))
same = True
for i, (x, y) in enumerate(zip(sa, sb)):
    name = names[i] if i < len(names) else str(i)
    if x == y:
        print("%-20s %5d kernels  identical" % (name, len(x)))
    else:
        same = False
        j = next((k for k in range(min(len(x), len(y))) if x[k] != y[k]), min(len(x), len(y)))
        print("%-20s %5d / %5d kernels  FIRST DIFFERENCE at %d:\n   A %s\n   B %s" % (name, len(x), len(y), j, x[j] if j < len(x) else None, y[j] if j < len(y) else None))
        print("   as multisets equal:", sorted(map(str, x)) == sorted(map(str, y)))
print("IDENTICAL" if same and len(sa) == len(sb) else "DIFFERENT")

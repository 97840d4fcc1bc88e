"""
Per-pass times of the pre-merge rounds from a kernel trace:
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/watershed_rate.py --premerge-only ...
    python tools/premerge_trace_summary.py DIR ROUNDS OUT.txt
Groups the trace's kernels by round (a round starts at choose and ends at the edge list's scan_assign) and
by call (ROUNDS rounds each), leaves the first call out as the warm-up and writes, per round and pass, the
number of launches and the median over the calls of the summed kernel time.
"""
import csv, glob, sys, collections, statistics
root, rounds, out = sys.argv[1], int(sys.argv[2]), sys.argv[3]
rows = []
for p in glob.glob(root + "/**/*kernel_trace.csv", recursive=True):
    with open(p) as f:
        rows += list(csv.DictReader(f))
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
KEYS = ("choose", "resolve", "double_parents", "set_min", "finish_map", "contract", "scan_count", "scan_block_sums",
        "scan_assign")
def short(name):
    if "exaspim" not in name:
        return None
    for key in KEYS:
        if "::" + key in name:
            if key in ("scan_count", "scan_assign"):
                return key + ("<SetHead>" if "SetHead" in name else "<UsedSlot>" if "UsedSlot" in name else "<other>")
            return key
    return None
# a round starts at choose and ends at the scan_assign<UsedSlot> after it
round_list, cur = [], None
for r in rows:
    s = short(r["Kernel_Name"])
    if s == "choose":
        cur = collections.OrderedDict()
        cur["_start"] = int(r["Start_Timestamp"])
    if cur is None or s is None or s.endswith("<other>"):
        continue
    if s == "scan_block_sums":
        s += "<SetHead>" if "scan_count<UsedSlot>" not in cur else "<UsedSlot>"
    a = cur.setdefault(s, [0, 0])
    a[0] += 1
    a[1] += int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
    if s == "scan_assign<UsedSlot>":
        cur["_end"] = int(r["End_Timestamp"])
        round_list.append(cur)
        cur = None
calls = [round_list[i:i + rounds] for i in range(0, len(round_list), rounds)]
timed = calls[1:]
with open(out, "w") as f:
    f.write(f"{len(calls)} calls of {rounds} rounds, the first one left out as the warm-up\n")
    for k in range(rounds):
        f.write(f"round {k + 1}\n")
        names = [n for n in timed[0][k] if not n.startswith("_")]
        total = []
        for n in names:
            ms = statistics.median(c[k][n][1] for c in timed) / 1e6
            f.write(f"  {n:28s} x{timed[0][k][n][0]:3d} {ms:8.3f} ms\n")
            total.append(ms)
        span = statistics.median(c[k]["_end"] - c[k]["_start"] for c in timed) / 1e6
        f.write(f"  sum {sum(total):8.3f} ms, choose's start to the last scan's end {span:8.3f} ms (memsets not in it)\n")
print(open(out).read())

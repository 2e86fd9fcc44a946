"""Share of the kernel time that the kernels whose name contains PATTERN take, from a rocprofv3 --kernel-trace --stats
`*_kernel_stats.csv`:  python3 scripts/kernel_share.py PATTERN stats.csv"""
import csv, sys
pattern, path = sys.argv[1], sys.argv[2]
rows = list(csv.DictReader(open(path)))
total = sum(float(r["TotalDurationNs"]) for r in rows)
hit = [r for r in rows if pattern in r["Name"]]
for r in hit:
    print(f"{r['Name'].split('(')[0]}: {r['Calls']} calls, {float(r['TotalDurationNs']) / 1e3:.1f} us in all, {float(r['AverageNs']) / 1e3:.2f} us each, "
          f"{100 * float(r['TotalDurationNs']) / total:.4f} % of the kernel time")
print(f"'{pattern}': {sum(float(r['TotalDurationNs']) for r in hit) / 1e3:.1f} us of {total / 1e6:.2f} ms kernel time = "
      f"{100 * sum(float(r['TotalDurationNs']) for r in hit) / total:.4f} %")

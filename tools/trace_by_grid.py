"""Launch statistics per (kernel, grid) of a `rocprofv3 --kernel-trace` run: a kernel name that serves several levels of the
network (instnorm_poolbwd_reduce, the weight gradients, k3pp_kernel) is one row in *_kernel_stats.csv; the grid tells the
levels apart.  usage: tools/trace_by_grid.py <rocprofv3 output dir> [kernel name regex]"""
import collections, csv, glob, re, sys
d = sys.argv[1]
pat = re.compile(sys.argv[2] if len(sys.argv) > 2 else "instnorm_poolbwd_reduce|deconv2_bwd_kernel|igemm_wgrad_kernel|k3pp_kernel")
f = glob.glob(d + "/*/*_kernel_trace.csv")
if not f:
    raise SystemExit("no kernel trace under " + d)
rows = list(csv.DictReader(open(f[0])))
agg = collections.defaultdict(list)
tot = 0.0
for r in rows:
    dur = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    tot += dur
    n = r["Kernel_Name"].replace("void (anonymous namespace)::", "").replace("(anonymous namespace)::", "")
    if pat.search(n):
        g = "x".join(str(r.get(k, "?")) for k in ("Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z"))   # in threads
        agg[(n[:90], g)].append(dur)
for (n, g), v in sorted(agg.items()):
    v2 = sorted(v)
    print(f"{len(v):5d} launches  mean {sum(v)/len(v):8.1f}  min {v2[0]:8.1f}  med {v2[len(v2)//2]:8.1f}  max {v2[-1]:8.1f} us  grid {g:>14s}  {n}")
print(f"all kernels: {tot/1e3:.3f} ms busy, {len(rows)} launches")

#!/usr/bin/env python3
"""Where the fixed cost of a K = 20 region goes: kernel dispatches and HIP runtime calls of one `bench.py --steps 20
--warmup 5` run on ONE time base (rocprofv3 --kernel-trace --hip-runtime-trace, csv).
   rocprofv3 --kernel-trace --hip-runtime-trace --output-format csv -d gpurun_out/prof_k20 -- \
       python3 bench.py --steps 20 --warmup 5 --no-cpu-baseline --no-single-queue-leg
   python3 tools/k20_trace.py gpurun_out/prof_k20
The timed region is found as the 20 fmi_kernel dispatches behind the longest launch-free gap that follows the settle
launches (the barrier in front of the region).

A long run (`--steps 1000 --warmup 100`) is reported by its steady state instead: for the largest dispatch group, per
queue the gap between the end of a dispatch and the start of the next one on the SAME queue, the start-to-start
interval over both queues, how many dispatches are in flight when one starts, and the HIP runtime calls the host makes
per step, by name (hipStreamWaitEvent / hipEventRecord are the lane's marker packets)."""
import csv, glob, os, sys
d = sys.argv[1]
kt = sorted(glob.glob(os.path.join(d, "*", "*kernel_trace.csv")), key=os.path.getmtime)[-1]
ht = sorted(glob.glob(os.path.join(d, "*", "*hip_api_trace.csv")), key=os.path.getmtime)[-1]
K = [r for r in csv.DictReader(open(kt)) if "fmi_kernel" in r["Kernel_Name"]]
K.sort(key=lambda r: int(r["Start_Timestamp"]))
st = [int(r["Start_Timestamp"]) for r in K]; en = [int(r["End_Timestamp"]) for r in K]
H = sorted(csv.DictReader(open(ht)), key=lambda r: int(r["Start_Timestamp"]))
launch = [r for r in H if "LaunchKernel" in r["Function"]]
# regions: groups of dispatches separated by an idle gap of > 30 us between one's end and the next one's start
groups, cur = [], [0]
for i in range(1, len(K)):
    if st[i] - max(en[:i][-3:]) > 30000: groups.append(cur); cur = []
    cur.append(i)
groups.append(cur)
print("dispatch groups (count):", [len(g) for g in groups][:12], "...")
for g in groups:
    if len(g) != 20: continue
    a, b = g[0], g[-1]
    t_first, t_last_end = st[a], max(en[i] for i in g)
    # the launch calls of this region: the 20 hipLaunchKernel calls that precede the dispatches
    ls = [r for r in launch if int(r["Start_Timestamp"]) < t_first + 2_000_000 and int(r["Start_Timestamp"]) > en[a - 1]]
    l0 = int(ls[0]["Start_Timestamp"]) if ls else None
    after = [r for r in H if int(r["End_Timestamp"]) > t_last_end][:4]
    print(f"region of 20 dispatches: first launch call -> first kernel start {(t_first - l0) / 1e3 if l0 else float('nan'):7.1f} us")
    print(f"   first kernel start -> last kernel end {(t_last_end - t_first) / 1e3:8.1f} us   (20 x steady step would be {20 * 46.85:.0f})")
    print("   start-to-start intervals (us):", " ".join(f"{(st[i + 1] - st[i]) / 1e3:.1f}" for i in g[:-1]))
    print("   durations (us):              ", " ".join(f"{(en[i] - st[i]) / 1e3:.1f}" for i in g))
    print("   last kernel end -> return of the call that sees it:")
    for r in after:
        print(f"      {r['Function']:28s} start {(int(r['Start_Timestamp']) - t_last_end) / 1e3:8.1f} us  end {(int(r['End_Timestamp']) - t_last_end) / 1e3:8.1f} us after the last kernel's end")
    if l0:
        print(f"   launch calls: the 20 take {(int(ls[min(19, len(ls) - 1)]['End_Timestamp']) - l0) / 1e3:.1f} us of host time")


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(q * len(v)))] if v else float("nan")


big = max(groups, key=len)
if len(big) >= 100:
    g = big[len(big) // 10: -len(big) // 10]            # the steady state: without the first and the last tenth
    q = [K[i].get("Queue_Id", "?") for i in g]
    print(f"steady state: {len(g)} of the {len(big)} dispatches of the largest group, queues {sorted(set(q))}")
    gaps = []
    last = {}
    for i, qi in zip(g, q):
        if qi in last: gaps.append((st[i] - en[last[qi]]) / 1e3)
        last[qi] = i
    s2s = [(st[g[j + 1]] - st[g[j]]) / 1e3 for j in range(len(g) - 1)]
    dur = [(en[i] - st[i]) / 1e3 for i in g]
    infl = [sum(1 for k in range(max(0, i - 4), i) if en[k] > st[i]) + 1 for i in g]
    for name, v in (("same-queue end -> start gap", gaps), ("start-to-start interval", s2s), ("dispatch duration", dur)):
        print(f"   {name:30s} us: median {pct(v, .5):7.2f}   p10 {pct(v, .1):7.2f}   p90 {pct(v, .9):7.2f}   mean {sum(v) / len(v):7.2f}")
    print(f"   dispatches in flight at a start (this one included): mean {sum(infl) / len(infl):.2f}, "
          + ", ".join(f"{n}: {infl.count(n)}" for n in sorted(set(infl))))
    t0, t1 = st[g[0]], st[g[-1]]
    # host calls are made ahead of the dispatches they cause: take the calls of the same span of launch calls
    lk = [r for r in launch if int(r["Start_Timestamp"]) < t1]
    lk = lk[-len(g):]
    h0, h1 = int(lk[0]["Start_Timestamp"]), int(lk[-1]["End_Timestamp"])
    calls = {}
    for r in H:
        if h0 <= int(r["Start_Timestamp"]) <= h1:
            c = calls.setdefault(r["Function"], [0, 0]); c[0] += 1; c[1] += int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
    print(f"   HIP runtime calls per step over the {len(lk)} launch calls in front of them (host span {(h1 - h0) / 1e3 / len(lk):.2f} us per step):")
    for fn, (n, ns) in sorted(calls.items(), key=lambda kv: -kv[1][0]):
        print(f"      {fn:28s} {n / len(lk):6.3f} per step   {ns / 1e3 / max(n, 1):7.2f} us each")
    marks = sum(n for fn, (n, _) in calls.items() if "WaitEvent" in fn or "EventRecord" in fn)
    print(f"   marker packets (event waits + records) per step: {marks / len(lk):.3f}")

"""Variant-coverage ledger: which kernel instantiations of libaether_hip.so a run dispatched.

    python3 tools/variant_coverage.py                                   # the library's kernels, by family
    python3 tools/variant_coverage.py --trace DIR [--out FILE] [--check] # against a rocprofv3 kernel trace

The list of kernels comes from the gfx950 code objects of the built library, as in tests/test_kernel_resources.py
(`llvm-objdump --offloading`, then `llvm-readelf -s` for the symbols and `-s -C` for the same symbols demangled, in the
same order): a kernel is a FUNC symbol that has a `<name>.kd` descriptor beside it.  The dispatches come from the
`*kernel_trace.csv` files of `rocprofv3 --kernel-trace --output-format csv -d DIR -- <command>` (every process of the
command, children included).  The report has four groups:
    dispatched                              library kernels the run launched (with the launch count)
    never dispatched                        library kernels the run did not launch, outside the allowlist
    never dispatched, allowlisted           the same, named in ALLOWLIST below with the reason no run can reach them
    dispatched, not in the library         a sanity check of the name matching (the HIP runtime's own copy and fill kernels land here)
--check exits 1 when a kernel of one of the CHECKED families is in the second group.
"""
import argparse
import collections
import csv
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
LIB = os.path.join(ROOT, "aether_primitives_amd", "lib", "libaether_hip.so")

# Families whose every instantiation must be dispatched by the suite or allowlisted (--check): the fused
# FFT*H*IFFT kernel, the element-wise kernels, the modulation kernels, the streamed power-of-two FFT and every kernel
# of the large-FFT planner's routes (tests/test_gpu_fft_routes.py).
CHECKED = ("fmi_kernel", "chain_kernel", "ew_kernel", "modulate_kernel", "modulate_generic_kernel",
           "modulate_awgn_kernel", "demod_kernel", "demod_generic_kernel", "fft_pow2_stream_kernel",
           "smallcol_kernel", "interleave_kernel", "transpose_kernel", "blu_pre", "blu_post", "blu_mul",
           "fourstep_rows", "fourstep_cols", "fft_ragged_kernel")

# (regex on the short name, why no test of `pytest -m gpu` reaches it).  "Not tested" is not a reason.
ALLOWLIST = [
    # lab-only: the plan routes 8192 points to its own row of the ragged table (aeth_fft.hip, aeth_fft_create); the
    # power-of-two stream build of 8192 runs only under AETH_FFT_NORAGGED=1, a knob of the lab build
    (r"^fft_pow2_stream_kernel<Cfg<8192,",
     "lab-only: 8192 points route to the ragged table; this build runs under AETH_FFT_NORAGGED=1 (lab build) only"),
    # unreachable: a chirp-z plan exists only for lengths that neither the power-of-two kernels nor the ragged table
    # serve, and every length up to 16 is served by one of them, so the one-launch convolution is never shorter than 64
    (r"^fmi_kernel<Cfg<(2|4|8|16|32), [^>]*>, true, 1, (true|false), true, 0>",
     "unreachable: chirp-z lengths start at 17 (2..16 are power-of-two or ragged rows), so M = pow2 >= 2n-1 >= 64"),
    # unreachable: split_fourstep_mixed (aeth_fft.hip) takes R = 2 only when len / 2 is register-resident.  len / 2 a
    # power of two makes len one (fourstep_pow2 or the single-workgroup kernels).  len / 2 a table row of at most 4096
    # points makes len <= 8192 with prime factors up to 23 (stockham_mixed, or a row itself).  The rows above 4096 are
    # the 5-smooth lengths up to 20480, so len is 5-smooth too: up to 20480 it is a row itself, and in (20480, 40960]
    # the first pass over the factors (rows of at most 8192 points) skips R = 2 and finds 5 or 10 (5 | len) or 6
    # (3 | len) before the second pass would try R = 2.  A brute-force mirror of the planner agrees for every length
    # up to 400000.
    (r"^(smallcol_kernel<2, |interleave_kernel<2, )",
     "unreachable: no length plans a first factor 2 (len / 2 register-resident makes len a power of two, a table "
     "row, a stockham_mixed length, or a length whose first pass finds R = 5, 6 or 10)"),
    # fourstep_pow2 (fft_plan_fourstep, aeth_fft_big.hip) splits 2^15 ... 2^24 into n1 = 128 (2^15, 2^23), 256 (2^16 ...
    # 2^19, 2^24), 512, 1024, 2048 (2^20 ... 2^22) columns over rows of n2 = 256 (2^15, 2^16), 512, 1024, 2048 (2^19 ...
    # 2^22) points or of 65536 (2^23, 2^24: a plan of their own, no row kernel).  AETH_POW2_SWITCH instantiates every
    # power of two 2 ... 4096 all the same; the other splits need AETH_4S_N1LOG / AETH_4S_DEEP_FROM, knobs of the lab build
    (r"^fourstep_cols<Cfg<(2|4|8|16|32|64|4096), ",
     "unreachable: fourstep_pow2 plans 128 ... 2048 columns only (other splits: AETH_4S_N1LOG, lab build)"),
    (r"^fourstep_rows<Cfg<(2|4|8|16|32|64|128|4096), ",
     "unreachable: fourstep_pow2 plans rows of 256 ... 2048 points, or 65536 as a sub-plan (other splits: AETH_4S_N1LOG, lab build)"),
    # launch_cols picks ONE column-group build per n1: 32 columns per workgroup where 32 * T lanes fit 1024 (n1 = 128,
    # 256), else 16; the ternary that picks it instantiates all three builds for every n1
    (r"^fourstep_cols<Cfg<(128|256), .*, 16, 1024>$",
     "lab-only: n1 <= 256 takes the 32-column build; the 16-column one runs under AETH_4S_COLG < 32 (lab build) only"),
    (r"^fourstep_cols<Cfg<(512|1024|2048), .*, 32, 1024>$",
     "unreachable: 32 columns of n1 >= 512 points exceed 1024 lanes (col_group_of < 32), so launch_cols never picks this build"),
    (r"^fourstep_cols<.*, 16, 512>$",
     "lab-only: the 512-lane column build runs under AETH_4S_MAXL <= 512 (lab build) only"),
]

# families with this many instantiations or more are summarised by count unless --full (the ragged FFT: one
# kernel per row of aeth_fft_ragged_table.inc)
COLLAPSE = 200


def short(name):
    """demangled kernel name -> compact form: no argument list, no namespaces, float2 / float4 for HIP_vector_type"""
    s = name.strip()
    if s.startswith("void "):
        s = s[5:]
    depth, cut = 0, len(s)
    for i, ch in enumerate(s):                   # the argument list: the first '(' at template depth 0 after the name
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0 and i > 0 and not s.startswith("(anonymous", i):
            cut = i
            break
    s = s[:cut]
    s = re.sub(r"HIP_vector_type<float, (\d)u>", r"float\1", s)
    s = s.replace("(anonymous namespace)::", "").replace("aeth::fftk::", "").replace("aeth::firk::", "").replace("aeth::", "")
    return re.sub(r">(?:\s+>)+", lambda m: m.group(0).replace(" ", ""), s)   # `> >` (libstdc++'s demangler) = `>>` (LLVM's)


def family(sname):
    return re.split(r"[<(]", sname, 1)[0]


def library_kernels(lib):
    """{demangled name: mangled name} of every kernel in the library's gfx950 code objects"""
    objdump, readelf = os.path.join(LLVM, "llvm-objdump"), os.path.join(LLVM, "llvm-readelf")
    out = {}
    with tempfile.TemporaryDirectory() as d:
        so = shutil.copy(lib, os.path.join(d, "lib.so"))
        subprocess.run([objdump, "--offloading", so], check=True, capture_output=True, cwd=d)
        for f in sorted(os.listdir(d)):
            if "gfx950" not in f:
                continue
            p = os.path.join(d, f)
            raw = subprocess.run([readelf, "-s", "-W", p], check=True, capture_output=True, text=True).stdout.splitlines()
            dem = subprocess.run([readelf, "-s", "-C", "-W", p], check=True, capture_output=True, text=True).stdout.splitlines()
            assert len(raw) == len(dem), f"{f}: llvm-readelf -s and -s -C disagree on the symbol count"
            names = set()
            rows = []
            for r, c in zip(raw, dem):
                fr, fc = r.split(), c.split(None, 7)
                if len(fr) < 8 or not fr[0].endswith(":"):
                    continue
                names.add(fr[7])
                rows.append((fr[3], fr[7], fc[7]))
            for typ, mangled, demangled in rows:
                if typ == "FUNC" and mangled + ".kd" in names:
                    out[demangled] = mangled
    return out


def dispatched_kernels(trace_dirs):
    """Counter {kernel name as the trace prints it: launches} over every kernel_trace.csv below the directories"""
    n = collections.Counter()
    files = []
    for d in trace_dirs:
        files += glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        sys.exit(f"no *kernel_trace.csv below {trace_dirs}")
    for f in files:
        with open(f, newline="") as fh:
            for row in csv.DictReader(fh):
                n[row["Kernel_Name"]] += 1
    return n, len(files)


def allow_reason(sname):
    for pat, why in ALLOWLIST:
        if re.search(pat, sname):
            return why
    return None


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", default=LIB)
    ap.add_argument("--trace", action="append", default=[], help="rocprofv3 output directory (repeatable)")
    ap.add_argument("--out", help="write the report here as well as to stdout")
    ap.add_argument("--title", default="", help="first line of the report")
    ap.add_argument("--full", action="store_true", help=f"list families of {COLLAPSE}+ instantiations kernel by kernel")
    ap.add_argument("--check", action="store_true", help="exit 1 if a CHECKED family has a never-dispatched kernel outside the allowlist")
    args = ap.parse_args()

    lib = library_kernels(args.lib)
    byshort = {}
    for dem in lib:
        byshort.setdefault(short(dem), []).append(dem)
    fams = collections.defaultdict(list)
    for s in sorted(byshort):
        fams[family(s)].append(s)

    lines = [args.title] if args.title else []
    lines.append(f"library: {len(lib)} kernels in {len(fams)} families (gfx950 code objects of {os.path.basename(args.lib)})")
    if not args.trace:
        for fam, ks in sorted(fams.items(), key=lambda kv: -len(kv[1])):
            lines.append(f"  {len(ks):5d}  {fam}")
        print("\n".join(lines))
        return 0

    disp, nfiles = dispatched_kernels(args.trace)
    count = collections.Counter()
    foreign = collections.Counter()
    for name, k in disp.items():
        s = short(name)
        if s in byshort:
            count[s] += k
        else:
            foreign[s] += k
    never, allowed = [], []
    for s in byshort:
        if count[s]:
            continue
        why = allow_reason(s)
        (allowed if why else never).append((s, why))
    lines.append(f"trace: {sum(disp.values())} dispatches of {len(disp)} kernels in {nfiles} kernel_trace.csv files")
    lines.append("")
    lines.append(f"{'family':32s} {'kernels':>8s} {'dispatched':>11s} {'never':>6s} {'allowlisted':>12s}")
    nv = collections.Counter(family(s) for s, _ in never)
    al = collections.Counter(family(s) for s, _ in allowed)
    for fam, ks in sorted(fams.items(), key=lambda kv: -len(kv[1])):
        d = sum(1 for s in ks if count[s])
        mark = "  *" if fam in CHECKED else ""
        lines.append(f"{fam:32s} {len(ks):8d} {d:11d} {nv[fam]:6d} {al[fam]:12d}{mark}")
    lines.append("(* = checked family: every instantiation dispatched or allowlisted)")

    def group(title, items, fmt):
        lines.append("")
        lines.append(f"== {title}: {len(items)}")
        byfam = collections.defaultdict(list)
        for it in items:
            byfam[family(it[0])].append(it)
        for fam in sorted(byfam):
            its = byfam[fam]
            if len(fams[fam]) >= COLLAPSE and not args.full:
                lines.append(f"  {fam}: {len(its)} of {len(fams[fam])} instantiations (listed with --full)")
                continue
            for it in sorted(its):
                lines.append("  " + fmt(it))

    group("dispatched", [(s, count[s]) for s in byshort if count[s]], lambda it: f"{it[1]:8d}  {it[0]}")
    group("never dispatched", never, lambda it: it[0])
    group("never dispatched, allowlisted", allowed, lambda it: f"{it[0]}\n      -- {it[1]}")
    lines.append("")
    lines.append(f"== dispatched, not in the library: {len(foreign)} ({sum(foreign.values())} dispatches)")
    for s, k in sorted(foreign.items()):
        lines.append(f"  {k:8d}  {s}")

    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)
    bad = [s for s, _ in never if family(s) in CHECKED]
    if args.check and bad:
        print(f"{len(bad)} never-dispatched kernels in checked families", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())

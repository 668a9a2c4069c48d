#!/usr/bin/env python3
"""Are the fmi_kernel builds of two revisions the same machine code?

    hipcc <the flags of csrc/Makefile for aeth_fir.hip> --cuda-device-only -S aeth_fir.hip -o old.s     (at the old revision)
    hipcc ...                                                               -o new.s                   (at the new one)
    tools/fmi_asm_diff.py [--family=SUBSTRING] old.s new.s [substring of a mangled name ...]

--family: the kernels compared are those whose mangled name contains SUBSTRING (default: fmi_kernel), so that other
families (corr_, stats_, levels_ ...) are checked with the same tool.

Every fmi_kernel instantiation present in both files is compared instruction by instruction after what a new neighbour
in the translation unit changes has been normalised away: comments, and the function's ordinal in its local labels
(.LBB94_7 -> .LBB_7).  A build whose only remaining differences are scalar loads of the HIDDEN kernel arguments (grid
size and the like, which sit behind the explicit ones), each moved by exactly the growth of FmiArgs, counts as
identical: that is the kernarg size and nothing else.  Prints one line per build that differs or whose name contains
one of the substrings, with the kernel descriptors' register counts, LDS and kernarg sizes, and a summary line.  A
function of the family without a kernel descriptor in either file ends the run with an error: every build counts."""
import hashlib
import re
import sys


def funcs(path):
    out, name, buf = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):\s", line)
        if m:
            name, buf = m.group(1), []
            out[name] = buf
            continue
        if name is not None:
            if line.startswith("\t.section") or line.startswith(".Lfunc_end"):
                name = None
                continue
            line = re.sub(r"\.LBB\d+_", ".LBB_", line.split(";")[0]).rstrip()
            if line:
                buf.append(line + "\n")
    return out


def meta(path):
    """{kernel: its descriptor fields} from amdhsa.kernels: a record opens with "  - .key:", its own keys are indented by
    four blanks (deeper ones belong to .args), and .name comes in the middle of them"""
    out, cur = {}, None
    keys = "name|vgpr_count|sgpr_count|vgpr_spill_count|private_segment_fixed_size|kernarg_segment_size|group_segment_fixed_size"
    for line in open(path):
        if line.startswith("  - ."):
            cur = {}
        m = re.match(r"(?:  - |    )\.(" + keys + r"):\s+(\S+)", line)
        if not m or cur is None:
            continue
        if m.group(1) == "name":
            out[m.group(2)] = cur
        else:
            cur[m.group(1)] = int(m.group(2))
    return out


def hidden_arg_moved(x, y, explicit_old, grow):
    """x, y: the same s_load of a kernel argument behind the explicit ones (256 bytes of hidden arguments follow them),
    y's offset larger by `grow`"""
    m, n = (re.match(r"(\ts_load_dword\w* s\S+ s\[\d+:\d+\], )(0x[0-9a-f]+)$", v.rstrip()) for v in (x, y))
    return bool(m and n and m.group(1) == n.group(1) and int(m.group(2), 16) >= explicit_old
                and int(n.group(2), 16) - int(m.group(2), 16) == grow)


def main():
    argv, family = sys.argv[1:], "fmi_kernel"
    if argv and argv[0].startswith("--family="):
        family, argv = argv[0].split("=", 1)[1], argv[1:]
    old, new, pats = argv[0], argv[1], argv[2:]
    a, b, ma, mb = funcs(old), funcs(new), meta(old), meta(new)
    same = diff = 0
    for k in sorted(a):
        if family not in k:
            continue
        if k not in b:
            print("ONLY IN OLD", k)
            continue
        if "kernarg_segment_size" not in ma.get(k, {}) or "kernarg_segment_size" not in mb.get(k, {}):
            sys.exit(f"{k}: in the family, without a kernel descriptor in {old if 'kernarg_segment_size' not in ma.get(k, {}) else new}")
        grow = mb[k]["kernarg_segment_size"] - ma[k]["kernarg_segment_size"]
        eq = len(a[k]) == len(b[k]) and all(x == y or hidden_arg_moved(x, y, ma[k]["kernarg_segment_size"] - 256, grow)
                                            for x, y in zip(a[k], b[k]))
        same += eq
        diff += not eq
        if not eq or any(p in k for p in pats):
            n = sum(1 for ln in a[k] if ln.startswith("\t") and not ln.startswith(("\t.", "\t;")))
            moved = sum(1 for x, y in zip(a[k], b[k]) if x != y) if eq else 0
            # hash of the code with the moved loads' offsets taken from the old build: equal hashes = the same code
            h = [hashlib.sha1("".join(x if eq and x != y else y for x, y in zip(a[k], other)).encode()).hexdigest()[:12]
                 for other in (a[k], b[k])]
            changed = {f: (ma[k].get(f), mb[k].get(f)) for f in ma.get(k, {}) if ma[k].get(f) != mb.get(k, {}).get(f)}
            print("IDENTICAL" if eq else "DIFFERENT", k, f"instructions {n}, sha1 {h[0]} / {h[1]}, hidden-argument loads moved: {moved};",
                  "descriptor:", ma.get(k),
                  "changed fields (old, new):", changed)
    added = len([k for k in b if family in k and k not in a])
    print(f"{family} builds in old: {same + diff}; identical code: {same}; different: {diff}; builds only in new: {added}")
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())

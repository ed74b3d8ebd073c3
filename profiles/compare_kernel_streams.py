#!/usr/bin/env python3
"""Compare the kernels of two gfx950 assembly listings (hipcc --cuda-device-only -S), kernel by kernel.

    python3 profiles/compare_kernel_streams.py parent/ip_kernels.s new/ip_kernels.s [--all]

Kernels are paired by demangled name.  Per kernel: instruction count, VGPRs, SGPRs (the total the compiler reports), scratch
bytes, LDS bytes, each as parent / new, and whether the instruction streams are identical once branch labels are renumbered
in order of appearance and comments are dropped.  Without --all only the kernels whose stream or counts differ are listed;
the summary line is always printed.  Exit status: 0 = same kernels on both sides (whatever their streams), 1 = a kernel
exists on one side only.  Reads the two files it is given and nothing else.
"""
import re
import shutil
import subprocess
import sys

LABEL = re.compile(r"\.L[A-Za-z_]+\d+(?:_\d+)?")
INFO = {"TotalNumSgprs": "sgpr", "NumVgprs": "vgpr", "ScratchSize": "scratch", "LDSByteSize": "lds"}


def parse(path):
    """name -> {"stream": [normalised instruction lines], "vgpr": .., "sgpr": .., "scratch": .., "lds": ..}"""
    functions, kernels, infos = {}, [], {}
    current = body = last_kernel = None
    with open(path, encoding="utf-8", errors="replace") as listing:
        for raw in listing:
            line = raw.rstrip("\n")
            begin = re.match(r"^([A-Za-z_$][\w$.]*):\s*; @\1\s*$", line)
            if begin:
                current, body = begin.group(1), []
                continue
            if current is not None:
                if re.match(r"^\.Lfunc_end\d+:", line):
                    functions[current] = body
                    current = None
                    continue
                code = line.split(";", 1)[0].strip()
                if not code or code.startswith(".section") or code.startswith(".p2align"):
                    continue
                if code.startswith(".amdhsa_kernel"):
                    last_kernel = code.split()[1]
                    kernels.append(last_kernel)
                    continue
                if code.startswith(".amdhsa_") or code.startswith(".end_amdhsa_kernel"):
                    continue
                body.append(code)
                continue
            info = re.match(r"^; (\w+): (\d+)", line)
            if info and info.group(1) in INFO and last_kernel is not None:
                infos.setdefault(last_kernel, {}).setdefault(INFO[info.group(1)], int(info.group(2)))
    out = {}
    for name in kernels:
        numbering = {}

        def renumber(match):
            return ".L%d" % numbering.setdefault(match.group(0), len(numbering))

        lines = [LABEL.sub(renumber, re.sub(r"\s+", " ", code)) for code in functions.get(name, [])]
        record = {"stream": lines, "count": sum(1 for l in lines if not l.endswith(":") and not l.startswith("."))}
        record.update(infos.get(name, {}))
        out[name] = record
    return out


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or shutil.which("/opt/rocm/llvm/bin/llvm-cxxfilt")
    names = list(names)
    if not tool or not names:
        return {n: n for n in names}
    text = subprocess.run([tool], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    plain = {}
    for mangled, long_name in zip(names, text):
        short = re.sub(r"^void ", "", long_name)
        short = short.replace("rp::(anonymous namespace)::", "").replace("rp::", "")
        cut, depth = len(short), 0      # drop the argument list: the template arguments tell the instantiations apart
        for at, ch in enumerate(short):
            depth += ch == "<"
            depth -= ch == ">"
            if ch == "(" and depth == 0:
                cut = at
                break
        plain[mangled] = short[:cut]
    return plain


def main(argv):
    show_all = "--all" in argv
    paths = [a for a in argv[1:] if a != "--all"]
    if len(paths) != 2:
        sys.stderr.write(__doc__)
        return 2
    sides = []
    for path in paths:
        parsed = parse(path)
        names = demangle(parsed)
        by_name = {}
        for mangled, record in parsed.items():
            key = names[mangled]
            if key in by_name:      # two kernels that differ in their arguments only: keep the mangled name apart
                key = names[mangled] + " [" + mangled + "]"
            by_name[key] = record
        sides.append(by_name)
    old, new = sides
    only_old, only_new = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    identical = differing = 0
    print("| kernel | instructions | VGPRs | SGPRs | scratch | LDS | identical stream |")
    print("|---|---|---|---|---|---|---|")
    for name in sorted(set(old) & set(new)):
        a, b = old[name], new[name]
        same = a["stream"] == b["stream"]
        identical += same
        differing += not same
        cells = ["%s / %s" % (a.get(k, "?"), b.get(k, "?")) for k in ("count", "vgpr", "sgpr", "scratch", "lds")]
        if show_all or not same or any(a.get(k) != b.get(k) for k in ("count", "vgpr", "sgpr", "scratch", "lds")):
            print("| `%s` | %s | %s |" % (name, " | ".join(cells), "yes" if same else "NO"))
    for name in only_old:
        print("only in %s: %s" % (paths[0], name))
    for name in only_new:
        print("only in %s: %s" % (paths[1], name))
    print("%d kernels paired: %d identical streams, %d differing; %d only in the first listing, %d only in the second"
          % (identical + differing, identical, differing, len(only_old), len(only_new)))
    return 1 if only_old or only_new else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))

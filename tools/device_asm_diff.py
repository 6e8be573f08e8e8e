#!/usr/bin/env python
"""Device assembly of two source trees, compared per device function.  Runs on any machine with hipcc; uses no GPU.

    git worktree add /tmp/parent HEAD~1          (or: git archive HEAD~1 | tar -x -C /tmp/parent)
    python tools/device_asm_diff.py /tmp/parent . [--jobs 8] [--markdown]

Every .hip file of each tree's stitching_amd/csrc is compiled with the command its own Makefile would run for it (`make -n`: FLAGS, EXTRA
and the per-file flag variable), with `--cuda-device-only -S` in place of `-c`.  A function is the text between its label and its
.Lfunc_end label, with comments and the numbers of local labels dropped (the function's index in its file is part of them); the
.amdhsa_kernel block of a kernel — registers, scratch, LDS — is compared with it.  A function of the first tree is looked for in the file
of the same name in the second tree, and, when it is not there, in the files only the second tree has: it must be there exactly once.
That is what a move of kernels between files has to show.  Exit status 1 when anything differs, is missing, doubled or new.
"""
import argparse
import concurrent.futures as cf
import os
import re
import shlex
import subprocess
import sys
import tempfile


def compile_commands(tree):
    """{file.hip: argv that writes the device assembly to argv[-1]} from the tree's own Makefile."""
    csrc = os.path.join(tree, "stitching_amd", "csrc")
    out = subprocess.run(["make", "-n", "-B", "-C", csrc, "OBJ=obj"], capture_output=True, text=True, check=True).stdout
    cmds = {}
    for line in out.splitlines():
        argv = shlex.split(line)
        if "-c" not in argv or not argv[argv.index("-c") + 1].endswith(".hip"):
            continue
        i = argv.index("-c")
        src = argv[i + 1]
        cmds[src] = argv[:i] + ["--cuda-device-only", "-S", src, "-o"]
    return csrc, cmds


def assemble(tree, tmp, jobs):
    csrc, cmds = compile_commands(tree)

    def run(item):
        src, argv = item
        dst = os.path.join(tmp, src[:-4] + ".s")
        r = subprocess.run(argv + [dst], cwd=csrc, capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit(f"{tree}: {src} does not compile\n{r.stderr[-2000:]}")
        return src, open(dst).read()

    with cf.ThreadPoolExecutor(jobs) as ex:
        return dict(ex.map(run, sorted(cmds.items())))


LOCAL = re.compile(r"\.L(BB|func_begin|func_end|tmp|JTI)\d+(_\d+)?")


def clean(lines):
    out = []
    for line in lines:
        line = line.split(";", 1)[0].rstrip()  # no ";" inside an operand of these listings
        line = LOCAL.sub(lambda m: ".L" + m.group(1) + (m.group(2) or ""), line)
        if line.strip():
            out.append(line)
    return "\n".join(out)


def functions(asm):
    """{name: (instructions, kernel descriptor or "")} of one assembly listing."""
    lines = asm.splitlines()
    names = [m.group(1) for m in (re.match(r"\s*\.type\s+(\S+),@function", ln) for ln in lines) if m]
    fns = {}
    for name in names:
        a = next(i for i, ln in enumerate(lines) if ln.startswith(name + ":"))
        b = next(i for i in range(a, len(lines)) if lines[i].startswith(".Lfunc_end"))
        desc = ""
        if f"\t.amdhsa_kernel {name}" in lines:
            k = lines.index(f"\t.amdhsa_kernel {name}")
            desc = clean(lines[k:lines.index("\t.end_amdhsa_kernel", k)])
        fns[name] = (clean(lines[a:b]), desc)
    return fns


def figures(desc):
    get = lambda key: (re.search(rf"\.amdhsa_{key}\s+(\S+)", desc) or [None, "-"])[1]
    return get("next_free_vgpr"), get("next_free_sgpr"), get("private_segment_fixed_size"), get("group_segment_fixed_size")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("first", help="source tree to compare against (the parent)")
    ap.add_argument("second", help="source tree under test")
    ap.add_argument("--jobs", type=int, default=max(1, min(8, os.cpu_count() or 1)))
    ap.add_argument("--markdown", action="store_true", help="print the table in markdown")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        A = {f: functions(s) for f, s in assemble(args.first, ta, args.jobs).items()}
        B = {f: functions(s) for f, s in assemble(args.second, tb, args.jobs).items()}
    new_files = [f for f in B if f not in A]
    used = set()
    rows, bad = [], []
    for f in sorted(A):
        where = {}  # file of the second tree -> [identical, differing]
        for name, body in A[f].items():
            hits = [f] if name in B.get(f, {}) else [g for g in new_files if name in B[g]]
            if len(hits) != 1:
                bad.append(f"{f}: {name} is in {len(hits)} files of the second tree {hits}")
                continue
            used.add((hits[0], name))
            same = B[hits[0]][name] == body
            where.setdefault(hits[0], [0, 0])[0 if same else 1] += 1
            if not same:
                what = "instructions" if B[hits[0]][name][0] != body[0] else "kernel descriptor"
                bad.append(f"{f} -> {hits[0]}: {name} differs ({what}; VGPRs, SGPRs, scratch, LDS {figures(body[1])} -> {figures(B[hits[0]][name][1])})")
        rows.append((f, len(A[f]), where))
    for g in sorted(B):
        for name in B[g]:
            if (g, name) not in used:
                bad.append(f"{g}: {name} is not in the first tree")
    sep = " | " if args.markdown else "  "
    edge = "| " if args.markdown else ""
    print(edge + sep.join(["file (first tree)", "functions", "identical", "found in (second tree)"]) + edge[::-1])
    if args.markdown:
        print("|---|---|---|---|")
    for f, n, where in rows:
        found = ", ".join(f"{g} {s + d}" for g, (s, d) in sorted(where.items()))
        print(edge + sep.join([f, str(n), str(sum(s for s, _ in where.values())), found]) + edge[::-1])
    total, same = sum(n for _, n, _ in rows), sum(s for _, _, w in rows for s, _ in w.values())
    print(f"\n{same} of {total} device functions identical (instructions and kernel descriptors); {len(bad)} findings")
    for b in bad:
        print("  " + b)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Do two trees compile the same kernels? For a split or a merge of translation units.

Compiles the named units of each tree device-only with the flags given after `--` (the unit's flags
of the Makefile; this tool keeps no flag list of its own), disassembles them and compares, kernel by
kernel under its demangled name: the instruction text with addresses stripped, and the register, LDS
and scratch figures of the code object's notes. What the layout of a code object decides is set
aside: the padding behind a function's last instruction, and the literal of the s_add_u32 /
s_addc_u32 that follow an s_getpc_b64 (the distance to a constant table or to a device function
that is called, not inlined); a kernel that differs only there is reported as `same/pcrel`.
Prints one line per kernel and exits 1 when a kernel is missing, doubled or different.

  python tools/isa_identity.py OLD_TREE NEW_TREE --old sdr_kernels.hip \\
      --new sdr_kernels.hip,sdr_ctx.hip,sdr_streams.hip,sdr_primitives.hip -- $HIPFLAGS -fno-slp-vectorize
"""
from __future__ import annotations

import argparse
import difflib
import hashlib
import pathlib
import re
import subprocess
import sys
import tempfile

LLVM = pathlib.Path("/opt/rocm/lib/llvm/bin")
CSRC = "real-time-sdr_amd/csrc"
FIGURES = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")
PADDING = ("...", "s_nop 0", "s_code_end")


def no_pcrel(lines: list[str]) -> list[str]:
    """the literals of the two adds behind each s_getpc_b64 masked"""
    out, left = [], 0
    for l in lines:
        if l.startswith("s_getpc_b64"):
            left = 2
        elif left and re.match(r"s_addc?_u32 ", l):
            l = re.sub(r"(0x[0-9a-f]+|-?\d+)$", "<pcrel>", l)
            left -= 1
        out.append(l)
    return out


def kernels(tree: pathlib.Path, unit: str, flags: list[str], tmp: str) -> dict[str, tuple[list[str], str]]:
    """demangled name -> (instructions, figures) of every function of the unit's code object"""
    obj = pathlib.Path(tmp) / (tree.name + "_" + unit + ".o")
    subprocess.run(["/opt/rocm/bin/hipcc", *flags, "-I", str(tree / "include"), "--cuda-device-only",
                    "--no-gpu-bundle-output", "-c", "-o", str(obj), str(tree / CSRC / unit)], check=True)
    run = lambda *a: subprocess.run(a, check=True, capture_output=True, text=True).stdout
    text: dict[str, list[str]] = {}
    cur = None
    for line in run(str(LLVM / "llvm-objdump"), "-d", "--demangle", "--no-show-raw-insn", str(obj)).split("\n"):
        m = re.match(r"^[0-9a-f]+ <(.*)>:$", line)
        if m:
            cur = text.setdefault(m.group(1), [])
        elif cur is not None and line.strip():
            # "  s_load_dwordx2 s[0:1], s[4:5], 0x0   // 000000001234: ..." -> no address comment
            cur.append(re.sub(r"\s*//.*$", "", line).strip())
    for t in text.values():
        while t and t[-1] in PADDING:
            t.pop()
    # the notes name kernels by their mangled symbols: the same listing without --demangle, in the same order
    mangled = re.findall(r"^[0-9a-f]+ <(.*)>:$", run(str(LLVM / "llvm-objdump"), "-d", "--no-show-raw-insn", str(obj)), re.M)
    demangle = dict(zip(mangled, text))
    figs: dict[str, str] = {}
    notes = run(str(LLVM / "llvm-readelf"), "--notes", str(obj))
    for blk in notes.split("  - .agpr_count:")[1:]:
        sym = re.search(r"\.symbol:\s+'?([^'\n]+?)\.kd'?\n", blk).group(1)
        figs[demangle[sym]] = " ".join(k[1:] + "=" + re.search(re.escape(k) + r":\s+(\d+)", blk).group(1) for k in FIGURES)
    return {n: (t, figs.get(n, "(device function)")) for n, t in text.items()}


def main() -> int:
    argv = sys.argv[1:]
    flags = argv[argv.index("--") + 1:] if "--" in argv else []
    ap = argparse.ArgumentParser()
    ap.add_argument("old_tree", type=pathlib.Path)
    ap.add_argument("new_tree", type=pathlib.Path)
    ap.add_argument("--old", required=True, help="units of the old tree, comma separated")
    ap.add_argument("--new", required=True, help="units of the new tree, comma separated")
    ap.add_argument("--show", type=int, default=12, help="changed lines printed per different kernel")
    args = ap.parse_args(argv[:argv.index("--")] if "--" in argv else argv)
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        old: dict[str, tuple[list[str], str]] = {}
        for u in args.old.split(","):
            old.update(kernels(args.old_tree.resolve(), u, flags, tmp))
        new: dict[str, list[tuple[str, tuple[list[str], str]]]] = {}
        for u in args.new.split(","):
            for n, v in kernels(args.new_tree.resolve(), u, flags, tmp).items():
                new.setdefault(n, []).append((u, v))
    for n in sorted(set(old) | set(new)):
        homes = new.get(n, [])
        changed: list[str] = []
        if n not in old:
            verdict = "NEW"
        elif not homes:
            verdict = "MISSING"
        elif len(homes) > 1:
            verdict = "TWICE"
        else:
            (t0, f0), (t1, f1) = old[n], homes[0][1]
            if f0 != f1:
                verdict = "DIFFERENT figures"
            elif t0 == t1:
                verdict = "same"
            elif no_pcrel(t0) == no_pcrel(t1):
                verdict = "same/pcrel"
                changed = [""] * sum(a != b for a, b in zip(t0, t1))
            else:
                verdict = "DIFFERENT instructions"
                changed = [l for l in difflib.unified_diff(no_pcrel(t0), no_pcrel(t1), "old", "new", lineterm="", n=0)
                           if l[0] in "+-" and l[:3] not in ("+++", "---")]
        bad += not verdict.startswith("same")
        t, f = old.get(n) or homes[0][1]
        note = f" ({len(changed)} pc-relative literals)" if verdict == "same/pcrel" else ""
        print(f"{verdict:10s} {','.join(u for u, _ in homes) or '-':18s} {len(t):5d} instr sha1 "
              f"{hashlib.sha1(chr(10).join(no_pcrel(t)).encode()).hexdigest()[:12]}  {f}  {n}{note}")
        if verdict.startswith("DIFFERENT"):
            print("".join(f"             {l}\n" for l in changed[:args.show]) + f"             ({len(changed)} changed lines)")
    print(f"{len(old)} functions in the old tree, {sum(len(h) for h in new.values())} in the new, {bad} not the same")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

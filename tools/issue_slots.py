#!/usr/bin/env python3
"""Static issue-slot report of k_search (CPU only).

With one wave per SIMD every instruction of k_search costs a full issue turn,
scalar ones, branches, waits and nops included (DESIGN.md §4 "Issue slots").
This compiles the search units to gfx950 assembly with build.py's flags plus
-S -DPOMCP_ASM_MARKS, picks the UCB / 256-lane kernels of both environments
and counts, per section between consecutive ;@@MARK comments (in text order)
and for the whole simulation loop (from the first mark 6 or 7, whichever the
compiler placed first, to the last mark 4), the instructions by mnemonic prefix.

"s.load" counts the scalar memory loads (s_load_dword*: a kernel argument or
a table word fetched again inside the loop, each followed by a wait that also
drains the LDS queue) and "v.rdlane" the v_readlane_b32 (a scalar read back
from an SGPR-spill lane), both part of their "s_" / "v.lane" columns.

usage: tools/issue_slots.py [--sections] [--dl 0 1 2 3] [--keep DIR] [--asm DIR]
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
from collections import Counter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "posggym-baselines_amd"))
from posggym_baselines_amd import build as B  # noqa: E402

KERNEL = re.compile(r"^(_Z\w*k_searchI\w*?Env(Driving|PursuitEvasion)ELi1ELi\d+ELi256ELi0E\w*):")
COLS = ("total", "v_", "v.f64", "v.cndmask", "v.cmp", "v.mov", "v.lane", "v.rdlane", "s_", "s.load",
        "s.saveexec", "s.branch", "s.waitcnt", "s.nop", "ds_", "global_", "other")


def classify(mn: str, c: Counter) -> None:
    c["total"] += 1
    if mn.startswith("v_"):
        c["v_"] += 1
        if "f64" in mn:
            c["v.f64"] += 1
        if "cndmask" in mn:
            c["v.cndmask"] += 1
        if mn.startswith("v_cmp"):
            c["v.cmp"] += 1
        if mn.startswith("v_mov"):
            c["v.mov"] += 1
        if mn.startswith(("v_readlane", "v_writelane")):
            c["v.lane"] += 1
        if mn.startswith("v_readlane"):
            c["v.rdlane"] += 1
    elif mn.startswith("s_"):
        c["s_"] += 1
        if mn.startswith("s_load_dword"):
            c["s.load"] += 1
        if "saveexec" in mn:
            c["s.saveexec"] += 1
        if mn.startswith(("s_cbranch", "s_branch")):
            c["s.branch"] += 1
        if mn.startswith("s_waitcnt"):
            c["s.waitcnt"] += 1
        if mn.startswith("s_nop"):
            c["s.nop"] += 1
    elif mn.startswith("ds_"):
        c["ds_"] += 1
    elif mn.startswith("global_"):
        c["global_"] += 1
    else:
        c["other"] += 1


def compile_asm(dl: int, out: str) -> None:
    src = B.SEARCH_DL_SOURCE if dl else B.SEARCH_SOURCE
    cmd = [B.HIPCC] + B.FLAGS + B.SEARCH_FLAGS + ["-S", "-DPOMCP_ASM_MARKS", "--cuda-device-only"]
    if dl:
        cmd.append(f"-DPB_SEARCH_DL={dl}")
    subprocess.run(cmd + ["-o", out, src], check=True)


def kernels(path: str):
    """(mangled name, env, [(mark or None, mnemonic), ...]) per selected kernel."""
    name, env, body = None, None, []
    with open(path) as f:
        for line in f:
            m = KERNEL.match(line)
            if m:
                name, env, body = m.group(1), m.group(2), []
                continue
            if name is None:
                continue
            t = line.strip()
            if t.startswith(";@@MARK"):
                body.append((int(t.split()[1]), None))
            elif t.startswith(".Lfunc_end"):
                yield name, env, body
                name = None
            elif t and t[0] not in ".;" and not t.split()[0].endswith(":"):
                body.append((None, t.split()[0]))


def report(name, env, body, sections: bool):
    marks = [i for i, (mk, _) in enumerate(body) if mk is not None]
    first = next(i for i in marks if body[i][0] in (6, 7))
    last = max(i for i in marks if body[i][0] == 4)
    rows = []
    loop = Counter()
    for _, mn in body[first:last]:
        if mn:
            classify(mn, loop)
    rows.append(("loop", loop))
    for a, b in zip(marks, marks[1:]):
        c = Counter()
        for _, mn in body[a:b]:
            if mn:
                classify(mn, c)
        rows.append((f"{body[a][0]}>{body[b][0]}", c))
    print(f"{env} {name}")
    print("  " + "section".ljust(8) + " ".join(k.rjust(10) for k in COLS))
    for label, c in rows if sections else rows[:1]:
        print("  " + label.ljust(8) + " ".join(str(c[k]).rjust(10) for k in COLS))
    sub = loop["s_"] + loop["other"]
    print(f"  loop scalar+branch+wait+nop: {sub} of {loop['total']}"
          f" (scalar ALU {loop['s_'] - loop['s.branch'] - loop['s.waitcnt'] - loop['s.nop']},"
          f" branches {loop['s.branch']}, waits {loop['s.waitcnt']}, nops {loop['s.nop']})")
    whole = Counter()
    for _, mn in body:
        if mn:
            classify(mn, whole)
    print(f"  kernel: {whole['total']} instructions, lane moves {whole['v.lane']},"
          f" saveexec in loop {loop['s.saveexec']}, s_load in loop {loop['s.load']},"
          f" v_readlane in loop {loop['v.rdlane']}")


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--dl", type=int, nargs="*", default=[1, 2, 3, 0])
    ap.add_argument("--sections", action="store_true", help="one row per section between marks")
    ap.add_argument("--keep", help="keep the assembly files in this directory")
    ap.add_argument("--asm", help="report the assembly files kept in this directory (no compile)")
    a = ap.parse_args()
    d = a.asm or a.keep or tempfile.mkdtemp()
    os.makedirs(d, exist_ok=True)
    for dl in a.dl:
        out = os.path.join(d, f"search_dl{dl}.s")
        if not a.asm:
            compile_asm(dl, out)
        print(f"== DL = {dl}" + (" (generic)" if dl == 0 else ""))
        for name, env, body in kernels(out):
            report(name, env, body, a.sections)


if __name__ == "__main__":
    main()

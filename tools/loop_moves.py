#!/usr/bin/env python3
"""Register moves inside the loops of the gfx950 kernels of libgoblin_hip.so, counted from the disassembly (no GPU).

    python tools/loop_moves.py [--json] [--kernel REGEX] [library]

The device images are found as tools/kernel_resources.py finds them and disassembled with the llvm-objdump that ships with
ROCm.  A loop is the address range [target, branch] of a backward branch (ranges with one target are merged).  Per kernel
and per loop: VALU instructions, plain register-to-register `v_mov_b32` (a VGPR source, no DPP / SDWA: the copies a phi or
an operand layout leaves behind), `v_readlane` / `v_writelane` (SGPR spill traffic and cross-lane reads) and `v_cndmask`.
`depth` is the number of loops around a loop, `parent` the index of the innermost of them (-1: none); a loop's counts
include the loops inside it, `own_*` leave them out.  The kernels on a VALU-issue bound pay for
every one of these in their traversal loops; tests/test_loop_moves_cpu.py holds the counts where the source has got them.
"""
import json
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_resources import FILT, device_images   # noqa: E402

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
SYM = re.compile(r"^([0-9a-f]+) <(.+)>:$")
INS = re.compile(r"^\s+(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):")
PLAIN_MOV = re.compile(r"^v\d+, v\d+$")
KEYS = ("valu", "mov", "lane", "cndmask")


def functions_of(image):
    """[(symbol, [(address, mnemonic, operands)])] of one device ELF."""
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(image)
        f.flush()
        text = subprocess.run([OBJDUMP, "-d", f.name], capture_output=True, text=True, check=True).stdout
    out = []
    for line in text.splitlines():
        m = SYM.match(line)
        if m:
            out.append((m.group(2), []))
            continue
        m = INS.match(line)
        if m and out:
            out[-1][1].append((int(m.group(3), 16), m.group(1), m.group(2)))
    return out


def classify(mn, ops):
    """Which of KEYS one instruction counts for."""
    if not mn.startswith("v_"):
        return ()
    kinds = ["valu"]
    if mn in ("v_mov_b32_e32", "v_mov_b32_e64", "v_mov_b32") and PLAIN_MOV.match(ops):
        kinds.append("mov")
    elif mn.startswith(("v_readlane", "v_writelane")):
        kinds.append("lane")
    elif mn.startswith("v_cndmask"):
        kinds.append("cndmask")
    return kinds


def loops_of(ins):
    """Backward branches -> [{start, end}] sorted by start, outer loops first; `ins` is one function's instruction list."""
    ext = {}
    for addr, mn, ops in ins:
        if mn.startswith(("s_cbranch_", "s_branch")) and re.fullmatch(r"\d+", ops):
            imm = int(ops)
            target = addr + 4 + 4 * (imm - 65536 if imm >= 32768 else imm)
            if target <= addr:
                ext[target] = max(ext.get(target, 0), addr)
    return [{"start": s, "end": e} for s, e in sorted(ext.items(), key=lambda se: (se[0], -se[1]))]


def count(ins, lo, hi, holes=()):
    c = dict.fromkeys(KEYS, 0)
    for addr, mn, ops in ins:
        if lo <= addr <= hi and not any(a <= addr <= b for a, b in holes):
            for k in classify(mn, ops):
                c[k] += 1
    return c


def kernel_row(symbol, ins):
    base = ins[0][0]
    loops = loops_of(ins)
    for i, lp in enumerate(loops):
        around = [j for j in range(i) if loops[j]["start"] <= lp["start"] and lp["end"] <= loops[j]["end"]]
        lp["depth"] = len(around)
        lp["parent"] = around[-1] if around else -1
    for i, lp in enumerate(loops):
        inner = [(l["start"], l["end"]) for l in loops if l["parent"] == i]
        lp.update(count(ins, lp["start"], lp["end"]))
        lp.update({"own_" + k: v for k, v in count(ins, lp["start"], lp["end"], inner).items()})
    for lp in loops:   # (offsets from the kernel's first instruction: they survive a relink)
        lp["start"] -= base
        lp["end"] -= base
    row = {"symbol": symbol, "instructions": len(ins), "loops": loops}
    row.update(count(ins, ins[0][0], ins[-1][0]))
    return row


def main():
    argv = sys.argv[1:]
    pattern = None
    if "--kernel" in argv:
        i = argv.index("--kernel")
        pattern = re.compile(argv[i + 1])
        del argv[i:i + 2]
    args = [a for a in argv if not a.startswith("--")]
    lib = args[0] if args else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "goblin_amd", "lib", "libgoblin_hip.so")
    funcs = []
    for img in device_images(open(lib, "rb").read()):
        funcs += [(s, ins) for s, ins in functions_of(img) if ins]
    names = subprocess.run([FILT], input="\n".join(s for s, _ in funcs), capture_output=True, text=True).stdout.splitlines()
    rows = []
    for (sym, ins), name in zip(funcs, names):
        if "rocprim" in name or (pattern is not None and not pattern.search(name)):
            continue
        row = kernel_row(sym, ins)
        row["name"] = name
        rows.append(row)
    if "--json" in sys.argv:
        print(json.dumps(rows, indent=1))
        return
    for r in sorted(rows, key=lambda r: r["name"]):
        print("%s\n  %-28s valu %5d  v_mov %4d  lane %4d  cndmask %4d" % (r["name"][:150], "whole (%d instructions)" % r["instructions"],
                                                                       r["valu"], r["mov"], r["lane"], r["cndmask"]))
        for i, lp in enumerate(r["loops"]):
            print("  %-28s valu %5d  v_mov %4d  lane %4d  cndmask %4d   own: valu %5d  v_mov %4d  lane %4d  cndmask %4d" % (
                "%s#%d +0x%x..+0x%x" % ("  " * lp["depth"], i, lp["start"], lp["end"]), lp["valu"], lp["mov"], lp["lane"], lp["cndmask"],
                lp["own_valu"], lp["own_mov"], lp["own_lane"], lp["own_cndmask"]))


if __name__ == "__main__":
    main()

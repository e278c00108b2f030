#!/usr/bin/env python
"""Per-kernel ISA table of the frame filters' kernel sources (runs on the CPU).

    python scripts/filter_isa.py [--root OTHER_CHECKOUT] [src.hip ...]

Cross-compiles each source (default: every csrc/denoise*_kernels.hip and csrc/temporal*_kernels.hip of the
checkout) for gfx950 with the library's flags and prints one line per kernel: VGPRs, SGPRs, scratch and LDS bytes
from the code-object metadata, the number of instructions, and a digest of the instruction stream (mnemonics and
operands in order; comments, directives and the function number inside branch labels left out).  Two kernels with
the same digest are the same instructions.  profiles/filter_refactor/isa.txt is this table for two checkouts.
"""
from __future__ import annotations

import argparse
import hashlib
import re
import subprocess
import sys
import tempfile
from pathlib import Path

FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-slp-vectorize",
         "-Wno-unused-function", "-mllvm", "-amdgpu-use-amdgpu-trackers=1", "--cuda-device-only", "-S"]
FIELDS = ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")


def kernels(text: str):
    """(symbol, instruction lines) of every kernel in the assembly text, (symbol -> metadata fields)."""
    meta = {}
    for ent in re.split(r"\n  - \.", text[text.index("amdhsa.kernels:"):])[1:]:
        name = re.search(r"\.name:\s+(\S+)", ent).group(1)
        meta[name] = {f: int(re.search(rf"\.{f}:\s+(\d+)", ent).group(1)) for f in FIELDS}
    for sym in meta:
        body = text[text.index(f"\n{sym}:") + 1:]
        body = body[:body.index(".Lfunc_end")]
        ins = []
        for ln in body.splitlines()[1:]:
            ln = re.sub(r"\.LBB\d+_", ".LBB_", ln.split(";")[0].strip())
            if ln and not (ln.startswith(".") and not ln.endswith(":")):
                ins.append(ln)
        yield sym, ins, meta[sym]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=str(Path(__file__).resolve().parent.parent))
    ap.add_argument("src", nargs="*")
    args = ap.parse_args()
    root = Path(args.root)
    csrc = root / "mirror-maze_amd" / "csrc"
    srcs = [Path(s) for s in args.src] or sorted([*csrc.glob("denoise*_kernels.hip"), *csrc.glob("temporal*_kernels.hip")])
    for src in srcs:
        with tempfile.TemporaryDirectory() as td:
            out = Path(td) / "k.s"
            subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, f"-I{root / 'include'}", f"-I{csrc}", "-o", str(out), str(src)],
                           check=True, stderr=subprocess.DEVNULL)
            text = out.read_text()
        for sym, ins, m in kernels(text):
            name = subprocess.run(["c++filt", sym], capture_output=True, text=True).stdout.strip()
            name = re.sub(r"mm::\(anonymous namespace\)::|^void ", "", name).split("(")[0]
            n = sum(1 for i in ins if not i.endswith(":"))
            digest = hashlib.sha1("\n".join(ins).encode()).hexdigest()[:12]
            print(f"vgpr {m['vgpr_count']:3d} sgpr {m['sgpr_count']:3d} scratch {m['private_segment_fixed_size']:3d} "
                  f"lds {m['group_segment_fixed_size']:3d} instructions {n:5d} stream {digest}  {src.name}: {name}")


if __name__ == "__main__":
    sys.exit(main())

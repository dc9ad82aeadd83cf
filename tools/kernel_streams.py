#!/usr/bin/env python3
"""One line per gfx950 kernel of the product's kernel translation units: a hash of its instruction stream (comments, directives and
blank lines dropped; labels kept), the instruction count, registers, scratch bytes and occupancy — from hipcc's device assembly with the
flags of vattention_amd/build.py.  No GPU needed.

Shows which BUILDS a source change touched:

    git stash            (or a checkout of the parent)
    python tools/kernel_streams.py > /tmp/before.txt
    git stash pop
    python tools/kernel_streams.py > /tmp/after.txt
    diff /tmp/before.txt /tmp/after.txt

A kernel whose line is unchanged kept its instruction stream.  Kernels are named by their mangled symbols (template arguments in
order: `Lin1E` is the decode kernels' ROPE = -1, the builds with the fused-rotary path compiled in).  `--units a.hip b.hip`: other translation units of vattention_amd/csrc."""
import argparse
import hashlib
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vattention_amd import build as B      # noqa: E402

UNITS = ("decode_kernels.hip", "prefill_kernels.hip", "prefill64_kernels.hip")
RES = ("TotalNumSgprs", "NumVgprs", "NumAgprs", "ScratchSize", "Occupancy")


def assembly(unit):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = ["--offload-arch=" + B.ARCH, "-O3", "-std=c++17", "-fPIC", "-pthread", "-Wno-inline-asm", *B.UNROLL_FLAGS]
    r = subprocess.run([hipcc, *flags, "-S", "--cuda-device-only", os.path.join(B.CSRC, unit), "-o", "-"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        sys.exit("hipcc failed on %s:\n%s" % (unit, r.stderr[-2000:]))
    return r.stdout


def kernels(text):
    """{symbol: (instruction lines, {resource: value})}"""
    out, name, body = {}, None, None
    for line in text.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, body = m.group(1), []
            out[name] = (body, {})
            continue
        if name is None:
            continue
        m = re.match(r"^; (\w+): (\d+)", line)
        if m and m.group(1) in RES:
            out[name][1][m.group(1)] = int(m.group(2))
        if body is None:
            continue
        t = line.split(";")[0].strip()
        if t.startswith(".Lfunc_end"):
            body = None
        elif t and (not t.startswith(".") or t.startswith(".LBB")):
            body.append(t)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--units", nargs="*", default=list(UNITS))
    a = ap.parse_args()
    with ThreadPoolExecutor(max_workers=len(a.units)) as ex:
        texts = list(ex.map(assembly, a.units))
    for unit, text in zip(a.units, texts):
        ks = kernels(text)
        for sym, (body, res) in sorted(ks.items()):
            h = hashlib.sha256("\n".join(body).encode()).hexdigest()[:16]
            print("%s  %s  instr=%d  %s  %s" % (unit, h, len(body), " ".join("%s=%s" % (k, res.get(k, "?")) for k in RES), sym))


if __name__ == "__main__":
    main()

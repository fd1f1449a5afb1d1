"""Scalar loads of the scheduled loop kernels (k_mpc_loop_sched<C>): the freshness check of DESIGN.md 3.2 / 3.3, redone from source.

    python tests/probes/mpc_sched_scalar_loads.py [--jobs 8] [--out profiles/mpc_log_scalar_loads.txt]

Compiles the device side of every scheduled-loop unit of the build (__graft_entry__.KERNEL_SETS) to assembly with the unit's own flags (hipcc
--cuda-device-only -S) and walks the body of every k_mpc_loop_sched kernel: each s_load_* / s_buffer_load_* is counted with the kind of
its offset operand -- an immediate, or a register.  The phases of the loop store with vector stores; what the solver reads after them
(scenario and LQR blocks, x0, x_1, the statistics) must therefore come through vector loads.  That holds if every scalar load of these
kernels reads the kernel-argument segment: an immediate offset below sizeof(MpcLoopSchedArgs) and no register offset, which would be
the sign of an indexed read of arena or block memory.  Prints the totals, the largest immediate and every kernel with a register offset;
exit status 1 if there is one or an immediate passes --segment."""
import argparse
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as G  # noqa: E402

LOAD = re.compile(r"^\s*(s_load_\w+|s_buffer_load_\w+)\s+(.*)$")
LABEL = re.compile(r"^(_Z\w+):")
IMM = re.compile(r"^(0x[0-9a-fA-F]+|\d+)$")


def assembly(unit, tmp):
    srcname, stem, extra = unit
    out = os.path.join(tmp, stem + ".s")
    flags = [f for f in G.compile_flags(unit) if f not in ("--offload-compress", "-fPIC")]
    subprocess.run(["/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"] + flags +
                   ["--cuda-device-only", "-S", os.path.join(G.CSRC, srcname), "-o", out], check=True, stderr=subprocess.DEVNULL)
    return out


def scan(path):
    """{kernel: [immediate loads, register-offset loads, largest immediate]}"""
    found, cur = {}, None
    for line in open(path):
        lab = LABEL.match(line)
        if lab:
            name = lab.group(1)
            cur = found.setdefault(name, [0, 0, 0]) if "k_mpc_loop_sched" in name else None
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
        m = LOAD.match(line) if cur is not None else None
        if not m:
            continue
        ops = [o.strip() for o in m.group(2).split(";")[0].split(",")]
        off = ops[2].split()[0] if len(ops) > 2 else "0"
        imm = re.search(r"offset:(0x[0-9a-fA-F]+|\d+)", m.group(2))
        if IMM.match(off):
            cur[0] += 1
            cur[2] = max(cur[2], int(off, 0))
        else:                                   # a register offset, with or without an immediate on top
            cur[1] += 1
            if imm:
                cur[2] = max(cur[2], int(imm.group(1), 0))
    return found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--segment", type=int, default=2560, help="sizeof(MpcLoopSchedArgs)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    units = G.KERNEL_SETS["sched"]
    kernels = {}
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(a.jobs) as ex:
        for path in ex.map(lambda u: assembly(u, tmp), units):
            kernels.update(scan(path))
    n_imm, n_reg, top = sum(k[0] for k in kernels.values()), sum(k[1] for k in kernels.values()), max(k[2] for k in kernels.values())
    lines = ["k_mpc_loop_sched kernels: %d in %d scheduled-loop units" % (len(kernels), len(units)),
             "scalar loads: %d, with an immediate offset %d (largest %d, kernel-argument segment %d bytes), with a register offset %d"
             % (n_imm + n_reg, n_imm, top, a.segment, n_reg)]
    lines += ["  register offset: %s (%d)" % (name, k[1]) for name, k in sorted(kernels.items()) if k[1]]
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if n_reg or top >= a.segment else 0


if __name__ == "__main__":
    sys.exit(main())

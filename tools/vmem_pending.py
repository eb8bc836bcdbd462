#!/usr/bin/env python3
"""Registers of in-flight loads, per kernel of the built libpdwt_hip.so (no GPU needed).

Loads written as inline asm (the hand-counted kernels: dwt_lat.hip, dwt_stream.hip, ...) are invisible to the compiler's wait insertion: once
the last consumer of a register has run, the compiler may give the register to other code while the load is still in flight, and the
load's data then lands on top of whatever was put there.  This walks a kernel's control-flow graph with the queue of outstanding vector
memory operations (vmcnt counts loads and stores in issue order on gfx9; `s_waitcnt vmcnt(N)` keeps the newest N) and reports every
instruction that reads or writes a register a pending load will still write.  Joins merge conservatively (a register pending on any path
stays pending).
usage: python tools/vmem_pending.py <kernel name prefix, mangled or as c++filt prints it> ..."""
import os
import re
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
REG = re.compile(r"\b([va])(?:(\d+)|\[(\d+):(\d+)\])")
VMEM = re.compile(r"^(global|buffer|flat|scratch)_(load|store|atomic)")


def _regs(s):
    out = set()
    for m in REG.finditer(s):
        if m.group(2) is not None:
            out.add((m.group(1), int(m.group(2))))
        else:
            out |= {(m.group(1), r) for r in range(int(m.group(3)), int(m.group(4)) + 1)}
    return frozenset(out)


def disassemble(lib=None):
    """{mangled kernel name: [(byte offset, opcode, operands, branch target offset or None)]} of every gfx950 kernel of the library."""
    lib = lib or os.path.join(ROOT, "pdwt_amd", "lib", "libpdwt_hip.so")
    data = open(lib, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    kernels = {}
    with tempfile.TemporaryDirectory() as td:
        i, n = 0, 0
        while True:
            i = data.find(magic, i)
            if i < 0:
                break
            q = i + len(magic)
            ne = struct.unpack_from("<Q", data, q)[0]
            q += 8
            for _ in range(ne):
                off, size, tl = struct.unpack_from("<QQQ", data, q)
                q += 24
                triple = data[q:q + tl].decode()
                q += tl
                if "gfx950" not in triple or size == 0:
                    continue
                path = os.path.join(td, "co_%03d.elf" % n)
                n += 1
                open(path, "wb").write(data[i + off:i + off + size])
                dis = subprocess.run([LLVM + "/llvm-objdump", "-d", "--no-show-raw-insn", path], capture_output=True, text=True).stdout
                name, base = None, 0
                for line in dis.split("\n"):
                    m = re.match(r"^([0-9a-f]+) <(\S+)>:", line)
                    if m:
                        name, base = m.group(2), int(m.group(1), 16)
                        kernels[name] = []
                        continue
                    m = re.match(r"^\s+(\S+)\s*(.*?)\s*//\s*([0-9A-F]+):", line)
                    if name is None or not m:
                        continue
                    tgt = re.search(r"<\S+\+0x([0-9a-f]+)>", line)
                    kernels[name].append((int(m.group(3), 16) - base, m.group(1), m.group(2), int(tgt.group(1), 16) if tgt else None))
            i += len(magic)
    return kernels


def pending_uses(ins):
    """[(byte offset, instruction, registers)] of the instructions that touch a register an outstanding load will still write."""
    idx = {ins[k][0]: k for k in range(len(ins))}

    def succ(k):
        off, op, args, tgt = ins[k]
        out = []
        if tgt is not None and (op == "s_branch" or op.startswith("s_cbranch")):
            out.append(idx.get(tgt))
        if op not in ("s_branch", "s_endpgm", "s_setpc_b64") and k + 1 < len(ins):
            out.append(k + 1)
        return [s for s in out if s is not None]

    def merge(a, b):
        if a is None:
            return b
        n = max(len(a), len(b))
        a2, b2 = (frozenset(),) * (n - len(a)) + a, (frozenset(),) * (n - len(b)) + b
        return tuple(x | y for x, y in zip(a2, b2))

    state, work, found = {0: ()}, [0], {}
    while work:
        k = work.pop()
        q = list(state[k])
        off, op, args, _ = ins[k]
        pend = frozenset().union(*q) if q else frozenset()
        if op == "s_waitcnt":
            m = re.search(r"vmcnt\((\d+)\)", args)
            if m:
                n = int(m.group(1))
                q = q[len(q) - n:] if n else []
        elif VMEM.match(op):
            ops = [o.strip() for o in args.split(",")]
            load = "_load" in op
            srcs = frozenset().union(*[_regs(o) for o in (ops[1:] if load else ops)]) if ops else frozenset()
            if srcs & pend:
                found.setdefault(off, (op + " " + args, sorted(srcs & pend)))
            q = (q + [_regs(ops[0]) if load else frozenset()])[-63:]
        elif _regs(args) & pend:
            found.setdefault(off, (op + " " + args, sorted(_regs(args) & pend)))
        nq = tuple(q)
        for s in succ(k):
            new = merge(state.get(s), nq)
            if new != state.get(s):
                state[s] = new
                work.append(s)
    return sorted((o, t, r) for o, (t, r) in found.items())


def demangle(names):
    """{mangled: name as tools/isa_audit.py prints it (c++filt, without `void pdwt::` and the argument list)}"""
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return {n: d.strip().split("(")[0].replace("void pdwt::", "") for n, d in zip(names, out)}


if __name__ == "__main__":
    ks = disassemble()
    dm = demangle(sorted(ks))
    for name in sorted(ks):
        if any(name.startswith(p) or dm[name].startswith(p) for p in sys.argv[1:]):
            hits = pending_uses(ks[name])
            print("%-60s %d" % (dm[name], len(hits)))
            for o, t, r in hits[:10]:
                print("    0x%x  %s   %s" % (o, t[:80], r[:4]))

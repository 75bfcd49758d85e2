"""Serial load-then-wait chains in the compiled kernels, read from the instruction stream.

    python tools/load_chains.py                      # the built libsndvae.so, the step's chain kernels
    python tools/load_chains.py --kernels 'zzt|dec'  # other kernels of the library (regex on the short name)
    python tools/load_chains.py FILE.s ...           # hipcc -S output instead of the library

Per kernel instantiation, in program order up to the first s_barrier and over the
whole kernel: the number of `s_waitcnt vmcnt(..)`, and how many of them follow one or
two vector-memory loads issued since the previous such wait (a wait with no load since
the last one only lowers the count on the same group: no new round trip).  A wait after one or two
loads is a memory round trip that hides almost nothing behind it; a kernel whose
time is one tile's dependent chain pays each of them in full.  Only loads, waits and
barriers are read: the counts say nothing about what the loads fetch.

    python tools/load_chains.py --args --kernels 'wgrad|reduce_kernel'

--args adds a second count per kernel, the scalar chain in front of the first vector-memory
instruction (load, store, atomic or LDS-DMA): the `s_waitcnt` carrying `lgkmcnt` that follow
at least one `s_load*` / `s_buffer_load*` issued since the previous such wait, and the
number of instructions up to that first vector-memory instruction.  Each such wait is one
dependent round trip to the kernel-argument segment (or to memory through a pointer taken
from it) that every workgroup pays before its first useful load.  The count is over the
program text, not over an execution: it includes the paths a given launch does not take
(both sides of a branch laid out before the first vector-memory instruction count), and
it stops at the first vector-memory instruction in text order even where a launch
branches round it.  With --args the kernel's VGPRs, SGPRs and `v_writelane` count (SGPR
spills into VGPR lanes) are printed when the input has them (hipcc -S files).
"""
import argparse
import os
import re
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJDUMP = os.environ.get("LLVM_OBJDUMP", "/opt/rocm/llvm/bin/llvm-objdump")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
# the shipped instantiations of the C2 step's chain kernels
DEFAULT = r"enc_front_kernel<2>|head_fwd_kernel<64, 2, 4>|head_bwd_kernel<128, 1, 2, 3>"

LOAD = re.compile(r"^(global_load|buffer_load|flat_load|scratch_load)")   # LDS-DMA forms included
VMEM = re.compile(r"^(global_|buffer_|flat_|scratch_)(load|store|atomic)")
SLOAD = re.compile(r"^s_(buffer_)?load")
LABEL_S = re.compile(r"^(_Z\w+):")                       # hipcc -S
LABEL_D = re.compile(r"^[0-9a-f]+ <(_Z\w+)>:")           # llvm-objdump -d


def code_objects(path):
    """The amdgcn code objects of every offload bundle in a host library or object."""
    with open(path, "rb") as f:
        d = f.read()
    out, at = [], d.find(MAGIC)
    while at >= 0:
        n, = struct.unpack_from("<Q", d, at + len(MAGIC))
        p = at + len(MAGIC) + 8
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", d, p)
            triple = d[p + 24:p + 24 + tl].decode()
            p += 24 + tl
            if "amdgcn" in triple and size:
                out.append(d[at + off:at + off + size])
        at = d.find(MAGIC, at + len(MAGIC))
    return out


def disassemble(lib):
    text = []
    for co in code_objects(lib):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            text.append(subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", f.name], check=True,
                                       capture_output=True, text=True).stdout)
    return "\n".join(text)


def kernels(text):
    """{mangled name: [instruction lines]} of a -S file or a disassembly."""
    out, cur = {}, None
    for line in text.splitlines():
        m = LABEL_S.match(line) or LABEL_D.match(line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        s = line.strip()
        if s.startswith(".Lfunc_end") or s.startswith(".end_amdhsa_kernel"):
            cur = None
        elif cur is not None and s and not s.startswith((";", ".", "//")):
            cur.append(s.split(";")[0].split("//")[0].strip())
    return out


def chains(insts):
    """Counts over one kernel's instructions: (waits, short waits) before the first
    barrier and in all, the loads before the first barrier, and the barriers."""
    r = {"waits_pre": 0, "short_pre": 0, "loads_pre": 0, "waits": 0, "short": 0, "loads": 0, "barriers": 0}
    since = 0
    for s in insts:
        pre = r["barriers"] == 0
        if s.startswith("s_barrier"):
            r["barriers"] += 1
        elif LOAD.match(s):
            since += 1
            r["loads"] += 1
            r["loads_pre"] += pre
        elif s.startswith("s_waitcnt") and "vmcnt(" in s:
            short = 1 <= since <= 2   # a lower count on the same group of loads is no new trip
            r["waits"] += 1
            r["short"] += short
            r["waits_pre"] += pre
            r["short_pre"] += short and pre
            since = 0
    return r


def arg_waits(insts):
    """The scalar chain in front of the first vector-memory instruction, in program order:
    waits on scalar loads (an lgkmcnt wait with at least one scalar load since the previous
    one), the scalar loads, and the instructions up to that vector-memory instruction; over
    the whole kernel, the v_writelane count.  Program text: untaken paths count too."""
    r = {"arg_waits": 0, "arg_loads": 0, "insts_to_vmem": 0, "writelanes": 0}
    since, front = 0, True
    for s in insts:
        if s.startswith("v_writelane"):
            r["writelanes"] += 1
        if not front:
            continue
        if VMEM.match(s):
            front = False
            continue
        r["insts_to_vmem"] += 1
        if SLOAD.match(s):
            since += 1
            r["arg_loads"] += 1
        elif s.startswith("s_waitcnt") and "lgkmcnt(" in s and since:
            r["arg_waits"] += 1
            since = 0
    return r


def registers(text):
    """{mangled name: (vgprs, sgprs)} from the .amdhsa directives of a hipcc -S file."""
    out, v = {}, {}
    for line in text.splitlines():
        m = re.match(r"\s*\.amdhsa_kernel (\S+)", line)
        if m:
            v = out.setdefault(m.group(1), {})
        m = re.match(r"\s*\.amdhsa_next_free_([vs])gpr (\d+)", line)
        if m:
            v[m.group(1)] = int(m.group(2))
    return out


def report_args(text, pattern):
    regs = registers(text)
    rows = {}
    for m, insts in kernels(text).items():
        name = short_name(m)
        if re.search(pattern, name):
            rows[name] = dict(arg_waits(insts), vgprs=regs.get(m, {}).get("v"), sgprs=regs.get(m, {}).get("s"))
    return rows


def format_args(rows):
    out = [f"{'kernel':44s} {'arg waits':>9s} {'s_loads':>7s} {'insts to vmem':>13s} | {'VGPRs':>5s} {'SGPRs':>5s} {'v_writelane':>11s}"]
    for name in sorted(rows):
        r = rows[name]
        reg = lambda k: f"{r[k]:5d}" if r.get(k) is not None else "    -"
        out.append(f"{name:44s} {r['arg_waits']:9d} {r['arg_loads']:7d} {r['insts_to_vmem']:13d} | "
                   f"{reg('vgprs')} {reg('sgprs')} {r['writelanes']:11d}")
    return "\n".join(out)


def short_name(mangled):
    """_ZN3snd12_GLOBAL__N_116enc_front_kernelILi2EEEvNS_9FrontArgsE -> enc_front_kernel<2>
    (nested names and integer template arguments: all this library's kernels have)"""
    m = re.match(r"_ZN?", mangled)
    p, name = m.end(), mangled
    while p < len(mangled) and mangled[p].isdigit():
        n = re.match(r"\d+", mangled[p:]).group(0)
        name = mangled[p + len(n):p + len(n) + int(n)]
        p += len(n) + int(n)
    if mangled[p:p + 1] == "I":
        targs = re.match(r"I((?:L[a-z]n?\d+E)+)E", mangled[p:])
        if targs:
            vals = re.findall(r"L[a-z](n?\d+)E", targs.group(1))
            name += "<" + ", ".join(v.replace("n", "-") for v in vals) + ">"
    return name


def report(text, pattern):
    ks = kernels(text)
    rows = {}
    for m, insts in ks.items():
        name = short_name(m)
        if re.search(pattern, name):
            rows[name] = chains(insts)
    return rows


def format_rows(rows):
    head = f"{'kernel':44s} {'pre: waits':>10s} {'short':>6s} {'loads':>6s} | {'all: waits':>10s} {'short':>6s} {'loads':>6s} {'barriers':>8s}"
    out = [head]
    for name in sorted(rows):
        r = rows[name]
        out.append(f"{name:44s} {r['waits_pre']:10d} {r['short_pre']:6d} {r['loads_pre']:6d} | "
                   f"{r['waits']:10d} {r['short']:6d} {r['loads']:6d} {r['barriers']:8d}")
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("files", nargs="*", help="hipcc -S outputs (default: disassemble --lib)")
    ap.add_argument("--lib", default=os.path.join(ROOT, "snd_vae_amd", "libsndvae.so"))
    ap.add_argument("--kernels", default=DEFAULT, help="regex on the kernel's short name, e.g. 'head_fwd_kernel<64, 2, 4>'")
    ap.add_argument("--args", action="store_true",
                    help="also the scalar-load waits in front of the first vector-memory instruction")
    args = ap.parse_args()
    if args.files:
        text = "\n".join(open(f).read() for f in args.files)
    else:
        text = disassemble(args.lib)
    rows = report(text, args.kernels)
    if not rows:
        sys.exit(f"no kernel matches {args.kernels!r}")
    print(format_rows(rows))
    if args.args:
        print()
        print(format_args(report_args(text, args.kernels)))


if __name__ == "__main__":
    main()

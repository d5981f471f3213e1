"""One line per kernel of the device side of zhip_lib.hip, made to be diffed between two trees. Analysis aid.
    name  instructions  vgprs  sgprs  scratch  lds  seq  bag  text
Instructions are the instruction lines between the kernel's label and its end; seq hashes the sequence of their mnemonics (first tokens), bag the
multiset of the mnemonics, text the lines themselves (comments and spacing dropped, the function's number taken out of block labels). It counts
and hashes; it looks for no particular instruction.
usage: python tests/tools/kernel_figures.py [file.s]      (without a file: compiles zhip_lib.hip to assembly as hot_loop_count.py does)"""
import hashlib, os, re, sys, tempfile
from hot_loop_count import compile_asm

INSTR = re.compile(r"\s+([a-z][a-z0-9_]*)\b\s*(.*)")
ENTRY = re.compile(r"  [ -] \.(name|vgpr_count|sgpr_count|private_segment_fixed_size|group_segment_fixed_size):\s+(\S+)")


def digest(items):
    return hashlib.sha1("\n".join(items).encode()).hexdigest()[:12]


def code(lines, kern):
    at = lines.index(next(l for l in lines if l.startswith(kern + ":")))
    ops = []
    for line in lines[at + 1:]:
        if line.startswith(".Lfunc_end"):
            return ops
        m = INSTR.match(line.split(";")[0].rstrip())
        if m:
            ops.append((m.group(1), re.sub(r"\.LBB\d+_", ".LBB_", " ".join(m.group(2).split()))))


with tempfile.TemporaryDirectory() as d:
    asm = sys.argv[1] if len(sys.argv) > 1 else os.path.join(d, "zhip_lib.s")
    if len(sys.argv) < 2:
        compile_asm(asm, [])
    lines = open(asm).read().split("\n")
kernels, cur = [], {}
for line in lines:                          # the .amdgpu_metadata document: an entry per kernel, "  - " in front of its first key
    if line.startswith("  - ."):
        cur = {}
        kernels.append(cur)
    m = ENTRY.match(line)
    if m:
        cur[m.group(1)] = m.group(2)
plain = lambda name: name[re.match(r"_Z\d+", name).end():][:int(re.match(r"_Z(\d+)", name).group(1))] if name.startswith("_Z") else name
print("%-44s %6s %5s %5s %7s %6s  %-12s %-12s %-12s" % ("kernel", "instr", "vgprs", "sgprs", "scratch", "lds", "seq", "bag", "text"))
for e in sorted((k for k in kernels if "name" in k), key=lambda k: plain(k["name"])):
    ops = code(lines, e["name"])
    print("%-44s %6d %5s %5s %7s %6s  %s %s %s" % (plain(e["name"]), len(ops), e["vgpr_count"], e["sgpr_count"], e["private_segment_fixed_size"], e["group_segment_fixed_size"],
                                                  digest([o for o, _ in ops]), digest(sorted(o for o, _ in ops)), digest(["%s %s" % o for o in ops])))

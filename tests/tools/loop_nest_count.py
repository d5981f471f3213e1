"""Static instruction count of a chosen loop nest of one kernel, by class. Analysis aid beside hot_loop_count.py, which picks the
innermost loop -- for K3 (zhip_decode_exec_kernel) that is not the batch loop: the batch loop is the largest loop at depth 2 (depth 1 is
the persistent wave's loop over frames), with the dependency rounds and the unit loops inside it.

The loops are the compiler's own: every basic block of the listing carries a comment that names the innermost loop it belongs to ("in Loop:
Header=BB28_4 Depth=1"), a loop header says "This Loop Header: Depth=2" and lists the loops inside it ("Child Loop BB28_98 Depth 3"). A nest
is a header at the given depth with all the loops inside it; a block counts for the nest its innermost loop belongs to, wherever the
compiler laid it out. Printed for the nests at that depth, largest first (--rank picks one; with a copy of K3's block code per literal mode
the kernel has one batch loop per copy): vector ALU, scalar (waits and nops listed again on their own), LDS, global, and the exec-mask nests
(s_and_saveexec and its kin: one per predicated region); and the kernel's registers, LDS and scratch from its .amdhsa directives.

usage: python tests/tools/loop_nest_count.py [kernel_name] [--depth 2] [--rank n | --all] [--asm file.s] [--keep file.s] [-- extra compiler flags]
       (kernel_name defaults to zhip_decode_exec_kernel; --all prints every nest at the depth that has inner loops)"""
import os, re, sys, tempfile
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hot_loop_count import INSTR, classify, compile_asm

RESOURCES = ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size")
BLOCK = re.compile(r"(?:\.L(BB[0-9_]+):|; %bb\.[0-9]+:)(.*)")
IN_LOOP = re.compile(r"in Loop: Header=(BB[0-9_]+) Depth=([0-9]+)")
HEADER = re.compile(r"This (?:Inner )?Loop Header: Depth=([0-9]+)")
CHILD = re.compile(r"Child Loop (BB[0-9_]+) Depth ([0-9]+)")


def raw_kernel_lines(path, kern):
    inside, out = False, []
    for line in open(path):
        if line.startswith(kern + ":"):
            inside = True
            continue
        if not inside:
            continue
        if line.startswith(".Lfunc_end"):
            return out
        out.append(line.rstrip("\n"))
    raise SystemExit("kernel %s not found in %s" % (kern, path))


def nests(lines, want_depth):
    """{header: [instructions]} for the loops at want_depth, inner loops folded into their nest"""
    owner = {}                     # loop header -> header of the nest at want_depth that holds it
    depth_of = {}
    ops_of = {}                    # innermost loop header -> its own blocks' instructions
    cur, label, opening = None, None, False
    for line in lines:
        m = BLOCK.match(line)
        if m:
            label, cur, opening = m.group(1), None, True
        elif not line.lstrip().startswith(";"):
            opening = False
        if opening:                # the label's line and the comment lines under it: which loop is the block in, which loops does it head
            il, hd, ch = IN_LOOP.search(line), HEADER.search(line), CHILD.search(line)
            if il: cur = il.group(1)
            if hd and label:
                cur = label; depth_of[label] = int(hd.group(1))
                if depth_of[label] == want_depth: owner[label] = label
            if ch and label and depth_of.get(label) == want_depth: owner[ch.group(1)] = label
            continue
        i = INSTR.match(line.split(";")[0])
        if i and cur is not None:
            ops_of.setdefault(cur, []).append((i.group(1), i.group(2)))
    out = {}
    for loop, ops in ops_of.items():
        if loop in owner: out.setdefault(owner[loop], []).extend(ops)
    inner = {h: sum(1 for l, o in owner.items() if o == h and l != h) for h in out}
    return out, inner


def resources(path, kern):
    """the .amdhsa_* values of the kernel's descriptor (behind `.amdhsa_kernel <name>`)"""
    out, inside = {}, False
    for line in open(path):
        s = line.strip()
        if s.startswith(".amdhsa_kernel"):
            inside = s.split()[1] == kern
        elif s.startswith(".end_amdhsa_kernel"):
            inside = False
        elif inside:
            for r in RESOURCES:
                if s.startswith(".amdhsa_" + r + " "):
                    out[r] = int(s.split()[1], 0)
    return out


def report(path, kern, want_depth, rank, every):
    found, inner = nests(raw_kernel_lines(path, kern), want_depth)
    order = sorted(found, key=lambda h: -len(found[h]))
    if every: order = [h for h in order if inner[h]]
    elif rank < len(order): order = [order[rank]]
    else: raise SystemExit("%s has %d loops at depth %d" % (kern, len(order), want_depth))
    for n, h in enumerate(order):
        c = classify(found[h])
        nest_count = sum(1 for op, _ in found[h] if op.endswith("_saveexec_b64"))
        print("%s, loop at %s (depth %d, %d loops inside%s): %d instructions" % (kern, h, want_depth, inner[h], ", number %d by size" % (n if every else rank), c["total"]))
        print("  vector ALU %d (DPP moves %d)" % (c["valu"], c["dpp_moves"]))
        print("  scalar     %d (s_waitcnt %d, s_nop %d)" % (c["scalar"], c["wait"], c["nop"]))
        print("  LDS        %d" % c["lds"])
        print("  global     %d" % c["glob"])
        print("  exec-mask nests %d" % nest_count)
    r = resources(path, kern)
    print("  kernel: " + "  ".join("%s %s" % (k, r.get(k, "?")) for k in RESOURCES))


def main(argv):
    extra = []
    if "--" in argv:
        k = argv.index("--")
        argv, extra = argv[:k], argv[k + 1:]
    asm = keep = None
    want_depth, rank, every, names = 2, 0, False, []
    it = iter(argv)
    for a in it:
        if a == "--asm": asm = next(it)
        elif a == "--keep": keep = next(it)
        elif a == "--depth": want_depth = int(next(it))
        elif a == "--rank": rank = int(next(it))
        elif a == "--all": every = True
        else: names.append(a)
    kern = names[0] if names else "zhip_decode_exec_kernel"
    if asm is None and keep:
        asm = keep
        compile_asm(asm, extra)
    if asm is not None:
        report(asm, kern, want_depth, rank, every)
    else:
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "zhip_lib.s")
            compile_asm(path, extra)
            report(path, kern, want_depth, rank, every)


if __name__ == "__main__":
    main(sys.argv[1:])

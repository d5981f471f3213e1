"""Static instruction count of one kernel's hot loop, by class. Analysis aid (a lone wave's time is its instruction count: DESIGN.md 4.1).

Compiles the device side of zhip_lib.hip to assembly with build.sh's flags (or reads an assembly file already made), takes the named
kernel, finds the innermost loop (a label with a backward branch to it and no such loop inside) that holds the most instructions and prints
how many of them are vector ALU, scalar (waits and nops included, and listed again on their own), LDS and global, plus the DPP moves that
are instructions of their own.

usage: python tests/tools/hot_loop_count.py [kernel_name] [--asm file.s] [--keep file.s] [-- extra compiler flags]
       (kernel_name defaults to zhip_decode_seq_kernel)"""
import os, re, subprocess, sys, tempfile

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "python-zstandard_amd", "csrc")


def compile_asm(out, extra):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-o", out, os.path.join(CSRC, "zhip_lib.hip")] + extra
    subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)


def kernel_lines(path, kern):
    inside, out = False, []
    for line in open(path):
        if line.startswith(kern + ":"):
            inside = True
            continue
        if not inside:
            continue
        if line.startswith(".Lfunc_end"):
            return out
        out.append(line.split(";")[0].rstrip())
    raise SystemExit("kernel %s not found in %s" % (kern, path))


INSTR = re.compile(r"\s+((?:v|s|ds|global|flat|buffer|scratch)_[a-z0-9_]+)\b(.*)")
LABEL = re.compile(r"(\.LBB[0-9_]+):")


def hot_loop(lines):
    at, ops = {}, []                        # label -> index into ops of the first instruction behind it
    for line in lines:
        m = LABEL.match(line)
        if m:
            at[m.group(1)] = len(ops)
            continue
        m = INSTR.match(line)
        if m:
            ops.append((m.group(1), m.group(2)))
    loops = []
    for i, (op, rest) in enumerate(ops):
        if op.startswith("s_cbranch") or op == "s_branch":
            t = rest.strip()
            if t in at and at[t] <= i:
                loops.append((at[t], i))
    inner = [l for l in loops if not any(o != l and l[0] <= o[0] and o[1] <= l[1] for o in loops)]
    if not inner:
        raise SystemExit("no loop found")
    lo, hi = max(inner, key=lambda l: l[1] - l[0])
    return ops[lo:hi + 1]


def classify(body):
    c = dict(total=len(body), valu=0, scalar=0, lds=0, glob=0, wait=0, nop=0, dpp_moves=0)
    for op, _ in body:
        if op.startswith("v_"):
            c["valu"] += 1
            if op.startswith("v_mov_b32_dpp"):
                c["dpp_moves"] += 1
        elif op.startswith("s_"):
            c["scalar"] += 1
            if op.startswith("s_waitcnt"):
                c["wait"] += 1
            elif op.startswith("s_nop"):
                c["nop"] += 1
        elif op.startswith("ds_"):
            c["lds"] += 1
        else:
            c["glob"] += 1
    return c


def main(argv):
    extra = []
    if "--" in argv:
        k = argv.index("--")
        argv, extra = argv[:k], argv[k + 1:]
    asm = keep = None
    names = []
    it = iter(argv)
    for a in it:
        if a == "--asm":
            asm = next(it)
        elif a == "--keep":
            keep = next(it)
        else:
            names.append(a)
    kern = names[0] if names else "zhip_decode_seq_kernel"
    if asm is None:
        if keep:
            asm = keep
            compile_asm(asm, extra)
        else:
            with tempfile.TemporaryDirectory() as d:
                asm = os.path.join(d, "zhip_lib.s")
                compile_asm(asm, extra)
                lines = kernel_lines(asm, kern)
            asm = None
    if asm is not None:
        lines = kernel_lines(asm, kern)
    c = classify(hot_loop(lines))
    print("%s hot loop: %d instructions" % (kern, c["total"]))
    print("  vector ALU %d (DPP moves %d)" % (c["valu"], c["dpp_moves"]))
    print("  scalar     %d (s_waitcnt %d, s_nop %d)" % (c["scalar"], c["wait"], c["nop"]))
    print("  LDS        %d" % c["lds"])
    print("  global     %d" % c["glob"])


if __name__ == "__main__":
    main(sys.argv[1:])

"""Kernel by kernel, the gfx950 disassembly and the code-object metadata of two builds of the product library (build container, no GPU): which kernels are the other
build's instruction for instruction, and VGPRs / SGPRs / spills / scratch / LDS / argument bytes of those that are not.  From every object file of both build
directories the code object is taken out (`llvm-objcopy --dump-section .hip_fatbin`, `clang-offload-bundler --unbundle`), disassembled (`llvm-objdump -d`), split per
kernel symbol, addresses and encodings dropped (a kernel that moves in the code object keeps its instructions), and compared under the demangled name without its
argument list (an argument added to a template changes every instantiation's symbol, not its code).
usage: python tools/diag/isa_compare.py PARENT_BUILD_DIR [BUILD_DIR] > report.txt     (build directories as `__graft_entry__.build()` leaves them: build/*.o)"""
import collections, os, re, subprocess, sys, tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def code_object(obj, out):
    subprocess.check_call([f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={out}.fatbin", obj, "/dev/null"], stderr=subprocess.DEVNULL)
    subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={out}.fatbin", f"--output={out}.co"])
    return out + ".co"


def kernels(co):
    d = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-leading-addr", "--no-show-raw-insn", co], capture_output=True, text=True, check=True).stdout
    ks, cur = collections.OrderedDict(), None
    for line in d.splitlines():
        m = re.match(r"^[0-9a-f]* ?<(.*)>:$", line)
        if m:
            cur = m.group(1); ks[cur] = []
        elif cur is not None and line.strip() and line.strip() != "...":  # ("...": the zero padding up to the next kernel's alignment, behind s_endpgm -- the last kernel of a code object has none)
            ks[cur].append(re.sub(r"\s+", " ", line.split("//")[0].strip()))  # (the comment holds the address and the encoding)
    return ks, len(d.splitlines())


def notes(co):
    t = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
    res = {}
    for blk in t.split("- .agpr_count")[1:]:
        g = lambda k: (re.search(rf"\.{k}:\s*(\S+)", blk) or [None, "?"])[1]
        res[g("name")] = dict(vgpr=g("vgpr_count"), sgpr=g("sgpr_count"), vgpr_spill=g("vgpr_spill_count"), sgpr_spill=g("sgpr_spill_count"), scratch=g("private_segment_fixed_size"),
                              lds=g("group_segment_fixed_size"), kernarg=g("kernarg_segment_size"))
    return res


def short(n):
    n = subprocess.run(["c++filt", n], capture_output=True, text=True).stdout.strip()
    return re.sub(r"\(.*$", "", re.sub(r"\(anonymous namespace\)::", "", n).replace("void ", ""))


def main():
    parent, now = sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "build")
    tmp = tempfile.mkdtemp()
    for f in sorted(os.listdir(now)):
        if not f.endswith(".o") or not os.path.exists(os.path.join(parent, f)):
            continue
        try:
            cp, cn = code_object(os.path.join(parent, f), os.path.join(tmp, "parent_" + f)), code_object(os.path.join(now, f), os.path.join(tmp, "now_" + f))
        except subprocess.CalledProcessError:
            print(f"## {f}: no device code"); continue
        (kp, lp), (kn, ln), np_, nn = kernels(cp), kernels(cn), notes(cp), notes(cn)
        print(f"## {f}: {lp} / {ln} lines of disassembly")
        sp, sn = {short(k): k for k in kp}, {short(k): k for k in kn}
        for s in sn:
            if s not in sp:
                print(f"   new        {s}\n        now    {nn.get(sn[s], {})}"); continue
            a, b = [x.replace(sp[s], "K") for x in kp[sp[s]]], [x.replace(sn[s], "K") for x in kn[sn[s]]]  # (branch targets carry the kernel's own symbol)
            print(f"   {'identical' if a == b else 'differs  '}  {s}" + ("" if a == b else f"  ({len(a)} -> {len(b)} instructions)"))
            if a != b:
                print(f"        parent {np_.get(sp[s], {})}\n        now    {nn.get(sn[s], {})}")
        for s in sp:
            if s not in sn:
                print(f"   gone       {s}")


if __name__ == "__main__":
    main()

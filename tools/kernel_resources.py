"""Print VGPR / scratch / LDS / occupancy per kernel from hipcc -Rpass-analysis=kernel-resource-usage output.

Usage: kernel_resources.py [--digest] [BUILD_DIR]      (BUILD_DIR: what `build.py --force --asm` filled)

--digest adds, per kernel, its LDS size, its instruction count and a SHA-256 of its instruction lines in the saved .s, and
prints the full demangled name last: two builds emit the same code for a kernel exactly when its two lines are equal.
Instruction lines are what is left of a function's body without directives, comments and blank lines; the function number
in local labels (.LBB<n>_<m>) is dropped, so a kernel's hash does not depend on its place in the file.
"""
import glob, hashlib, os, re, subprocess, sys

args = [a for a in sys.argv[1:] if a != "--digest"]
digest = "--digest" in sys.argv[1:]
d = args[0] if args else "vae-posterior-consistency_amd/csrc/build"


def instruction_lines(asm_path):
    """{symbol: [instruction and label lines of its body]} for every function of a device .s file"""
    out, name, body = {}, None, []
    for line in open(asm_path):
        line = line.split(";", 1)[0].strip()
        if not line:
            continue
        if name is None:
            m = re.fullmatch(r"([A-Za-z_][\w$.]*):", line)
            if m:
                name, body = m.group(1), []
        elif line.startswith(".Lfunc_end"):
            out[name], name = body, None
        elif not line.startswith(".") or line.endswith(":"):
            body.append(re.sub(r"\.L([A-Za-z]+)\d+_", r".L\1_", line))
    return out


for f in sorted(glob.glob(os.path.join(d, "*.resource.txt"))):
    txt = open(f).read()
    asm = f[:-len(".o.resource.txt")] + "-hip-amdgcn-amd-amdhsa-gfx950.s"
    bodies = instruction_lines(asm) if digest else {}
    for blk in txt.split("Function Name:")[1:]:
        name = blk.split()[0]
        dem = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
        g = lambda k: re.search(re.escape(k) + r":\s*(\d+)", blk)
        vals = {k: (g(k).group(1) if g(k) else "?") for k in
                ["VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs", "LDS Size [bytes/block]"]}
        short = re.sub(r"vpc::|\(vpc::\w+\)", "", dem)
        res = f"vgpr={vals['VGPRs']:>4} agpr={vals['AGPRs']:>4} sgpr={vals['SGPRs']:>4} scratch={vals['ScratchSize [bytes/lane]']:>5} occ={vals['Occupancy [waves/SIMD]']}"
        if not digest:
            print(f"{short[:70]:70s} {res}")
            continue
        body = bodies[name]
        insts = [l for l in body if not l.endswith(":")]
        sha = hashlib.sha256("\n".join(body).encode()).hexdigest()
        print(f"{res} lds={vals['LDS Size [bytes/block]']:>6} insts={len(insts):>6} sha256={sha}  {short}")

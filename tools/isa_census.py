"""Instruction census of the device assembly that `python build.py --asm` leaves in csrc/build/.

Usage: isa_census.py [--filter SUBSTRING] [BUILD_DIR | FILE.s ...]

Per kernel symbol: the counts of MFMA, of VALU in four categories (int/address, moves, select/compare, float), of ds_* and
of vector memory instructions, for the whole function and - where a loop can be delimited by its labels - for the tile-pass
loop: the shortest span from a local label to a later branch back to it that holds as many MFMAs as any such span of the
function (the pass loop of the MFMA kernels; the persistent tile loop around it adds no MFMA).  A histogram by opcode prefix
and nothing else: it says what is issued, not what it costs.
"""
import collections
import glob
import os
import re
import subprocess
import sys

INT = ("v_add_u32", "v_add_i32", "v_sub_u32", "v_subrev_u32", "v_sub_i32", "v_add_co", "v_addc_co", "v_sub_co", "v_subb_co",
       "v_subrev_co", "v_add3_u32", "v_lshl", "v_lshr", "v_ashr", "v_and_b32", "v_or_b32", "v_xor_b32", "v_not_b32", "v_and_or_b32",
       "v_or3_b32", "v_xad_u32", "v_add_lshl_u32", "v_mul_lo", "v_mul_hi", "v_mul_u32", "v_mul_i32", "v_mad_u32", "v_mad_i32",
       "v_mad_u64", "v_mad_i64", "v_min_u32", "v_max_u32", "v_min_i32", "v_max_i32", "v_alignbit", "v_alignbyte", "v_perm_b32",
       "v_bcnt", "v_mbcnt", "v_ffbh", "v_ffbl", "v_pk_add_u16", "v_pk_lshl", "v_pk_lshr")
MOVE = ("v_mov_b", "v_readlane", "v_readfirstlane", "v_writelane", "v_accvgpr", "v_swap", "v_permlane", "v_movrel")
SEL = ("v_cndmask", "v_cmp", "v_bfe", "v_bitop3", "v_bfi")
COLS = ["mfma", "int/addr", "moves", "sel/cmp", "float", "valu", "ds", "vmem"]


def classify(op):
    if op.startswith("v_mfma") or op.startswith("v_smfma"):
        return "mfma"
    if op.startswith("ds_"):
        return "ds"
    if op.startswith(("buffer_", "global_", "flat_", "scratch_")):
        return "vmem"
    if not op.startswith("v_"):
        return None
    if op.startswith(MOVE):
        return "moves"
    if op.startswith(SEL):
        return "sel/cmp"
    if op.startswith(INT):
        return "int/addr"
    return "float"


def functions(path):
    """{symbol: [stripped lines of the body, labels included]} for every function of a device .s file"""
    out, name, body = {}, None, []
    for line in open(path):
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
            body.append(line)
    return out


def count(lines):
    c = collections.Counter()
    for l in lines:
        if l.endswith(":"):
            continue
        k = classify(l.split()[0])
        if k:
            c[k] += 1
    c["valu"] = c["int/addr"] + c["moves"] + c["sel/cmp"] + c["float"]
    return c


def pass_loop(body):
    """(first, last) line index of the tile-pass loop, or None"""
    label_at = {l[:-1]: i for i, l in enumerate(body) if l.endswith(":")}
    spans = []
    for i, l in enumerate(body):
        m = re.match(r"s_c?branch\w*\s+(\S+)", l)
        if m and m.group(1) in label_at and label_at[m.group(1)] < i:
            spans.append((label_at[m.group(1)], i))
    if not spans:
        return None
    mf = [count(body[a:b + 1])["mfma"] for a, b in spans]
    best = max(mf)
    if best == 0:
        return None
    return min((s for s, n in zip(spans, mf) if n == best), key=lambda s: s[1] - s[0])


def row(tag, c):
    return f"  {tag:14s}" + "".join(f" {c[k]:>8d}" for k in COLS)


def main(argv):
    flt = None
    if "--filter" in argv:
        i = argv.index("--filter")
        flt = argv[i + 1]
        argv = argv[:i] + argv[i + 2:]
    paths = []
    for a in argv or ["vae-posterior-consistency_amd/csrc/build"]:
        paths += sorted(glob.glob(os.path.join(a, "*-hip-amdgcn-amd-amdhsa-gfx950.s"))) if os.path.isdir(a) else [a]
    print(f"  {'':14s}" + "".join(f" {k:>8s}" for k in COLS))
    for p in paths:
        for name, body in functions(p).items():
            dem = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip() or name
            short = re.sub(r"vpc::|\(vpc::\w+\)", "", dem)
            if flt and flt not in short:
                continue
            print(f"{os.path.basename(p).split('-hip-')[0]}: {short}")
            print(row("whole function", count(body)))
            span = pass_loop(body)
            if span:
                print(row("tile-pass loop", count(body[span[0]:span[1] + 1])))


if __name__ == "__main__":
    main(sys.argv[1:])

"""tools/isa_census.py and tools/mfma_waits.py for a kernel that runs several tile loops one after the other (the phases of
step_f32_kernel, csrc/vpc_step_f32.hip): the function is cut at its outermost loops that hold MFMAs, and each gets the census of
its tile-pass loop and the MFMA / LDS-wait statistics, as the two tools print them for a kernel with one loop.

Usage: phase_census.py --filter SUBSTRING [BUILD_DIR | FILE.s ...]
"""
import collections
import glob
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_census as ic  # noqa: E402


def outer_loops(body):
    """(first, last) of every loop with MFMAs that lies in no other loop"""
    label_at = {l[:-1]: i for i, l in enumerate(body) if l.endswith(":")}
    spans = []
    for i, l in enumerate(body):
        m = re.match(r"s_c?branch\w*\s+(\S+)", l)
        if m and m.group(1) in label_at and label_at[m.group(1)] < i:
            spans.append((label_at[m.group(1)], i))
    spans = [s for s in spans if ic.count(body[s[0]:s[1] + 1])["mfma"]]
    return sorted(s for s in spans if not any(o != s and o[0] <= s[0] and s[1] <= o[1] for o in spans))


def waits(lines):
    lines = [l for l in lines if not l.endswith(":")]
    mf = [l for l in lines if l.startswith("v_mfma")]
    same = sum(1 for a, b in zip(mf, mf[1:]) if a.split()[1] == b.split()[1])
    hist = collections.Counter()
    for k in range(2, len(lines)):
        m = re.search(r"lgkmcnt\((\d+)\)", lines[k - 1]) if lines[k - 1].startswith("s_waitcnt") else None
        if m and lines[k].startswith("v_mfma"):
            hist[(int(m.group(1)), lines[k - 2].startswith("ds_read"))] += 1
    out = [f"    MFMAs {len(mf)}, successive pairs on one accumulator {same}"]
    for (n, ds), v in sorted(hist.items()):
        out.append(f"    MFMA groups behind lgkmcnt({n}){', directly behind a ds_read' if ds else ''}: {v}")
    return out


def main(argv):
    i = argv.index("--filter")
    flt, argv = argv[i + 1], argv[:i] + argv[i + 2:]
    paths = []
    for a in argv or ["vae-posterior-consistency_amd/csrc/build"]:
        paths += sorted(glob.glob(os.path.join(a, "*-hip-amdgcn-amd-amdhsa-gfx950.s"))) if os.path.isdir(a) else [a]
    print(f"  {'':14s}" + "".join(f" {k:>8s}" for k in ic.COLS))
    for p in paths:
        for name, body in ic.functions(p).items():
            dem = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip() or name
            short = re.sub(r"vpc::|\(vpc::\w+\)", "", dem)
            if flt not in short:
                continue
            print(f"{os.path.basename(p).split('-hip-')[0]}: {short}")
            print(ic.row("whole function", ic.count(body)))
            for n, (a, b) in enumerate(outer_loops(body)):
                seg = body[a:b + 1]
                span = ic.pass_loop(seg) or (0, len(seg) - 1)
                loop = seg[span[0]:span[1] + 1]
                print(ic.row(f"loop {n}", ic.count(loop)))
                print("\n".join(waits(loop)))


if __name__ == "__main__":
    main(sys.argv[1:])

"""How the MFMA groups of a kernel's tile-pass loop meet their LDS operands, from the device assembly `python build.py --asm` leaves
in csrc/build/.

Usage: mfma_waits.py --filter SUBSTRING [BUILD_DIR | FILE.s ...]

Per kernel symbol, inside the loop tools/isa_census.py delimits: the MFMAs, the successive MFMA pairs that write the same
accumulator (a dependent chain: 40 cycles of latency against 32 of issue for v_mfma_f32_16x16x4_f32), and the MFMAs that
directly follow an `s_waitcnt lgkmcnt(N)`, by N and by whether the instruction in front of the wait is a ds_read - N = 0
directly behind a ds_read is a fragment requested immediately before the MFMAs that use it, behind a full LDS wait.
"""
import collections
import glob
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_census as ic  # noqa: E402


def main(argv):
    i = argv.index("--filter")
    flt, argv = argv[i + 1], argv[:i] + argv[i + 2:]
    paths = []
    for a in argv or ["vae-posterior-consistency_amd/csrc/build"]:
        paths += sorted(glob.glob(os.path.join(a, "*-hip-amdgcn-amd-amdhsa-gfx950.s"))) if os.path.isdir(a) else [a]
    for p in paths:
        for name, body in ic.functions(p).items():
            dem = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip() or name
            short = re.sub(r"vpc::|\(vpc::\w+\)", "", dem)
            span = ic.pass_loop(body)
            if flt not in short or not span:
                continue
            lines = [l for l in body[span[0]:span[1] + 1] if not l.endswith(":")]
            mf = [l for l in lines if l.startswith("v_mfma")]
            same = sum(1 for a, b in zip(mf, mf[1:]) if a.split()[1] == b.split()[1])
            hist = collections.Counter()
            for k in range(2, len(lines)):
                m = re.search(r"lgkmcnt\((\d+)\)", lines[k - 1]) if lines[k - 1].startswith("s_waitcnt") else None
                if lines[k].startswith("v_mfma") and m:
                    hist[(int(m.group(1)), lines[k - 2].startswith("ds_read"))] += 1
            print(short)
            print(f"  MFMAs {len(mf)}, successive pairs on one accumulator {same}")
            for (n, behind), cnt in sorted(hist.items()):
                print(f"  MFMA groups behind lgkmcnt({n}){', directly behind a ds_read' if behind else ''}: {cnt}")


if __name__ == "__main__":
    main(sys.argv[1:])

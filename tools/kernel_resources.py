"""Kernel resource table from hipcc's -Rpass-analysis=kernel-resource-usage remarks, one or two builds side by side.

  hipcc --offload-arch=gfx950 -O3 -std=c++17 -mllvm -amdgpu-mfma-vgpr-form=1 -fPIC --cuda-device-only -S \
        -Rpass-analysis=kernel-resource-usage FILE.hip -o FILE.s 2> FILE.remarks
  python3 tools/kernel_resources.py PARENT.remarks [CHANGE.remarks] [--match SUBSTRING ...]

Columns per build: VGPRs, SGPRs, scratch bytes per lane, LDS bytes per block, waves per SIMD.  With two files every
kernel of either is listed, a `!=` marks a row whose figures differ, and the last line counts them.  CPU only."""
import re
import subprocess
import sys

FIELDS = [("VGPRs", "vgpr"), ("TotalSGPRs", "sgpr"), ("ScratchSize [bytes/lane]", "scratch"),
          ("LDS Size [bytes/block]", "lds"), ("Occupancy [waves/SIMD]", "occ")]


def parse(path):
    out, name = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark:\s+(.*?): (\S+) \[-Rpass-analysis", line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            name = val
            out[name] = {}
        elif name:
            for field, short in FIELDS:
                if key == field:
                    out[name][short] = int(val)
    return out


def demangle(names):
    res = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    short = [re.sub(r"\(anonymous namespace\)::|\(.*$|^void ", "", s) for s in res.stdout.splitlines()]
    return dict(zip(names, short))


def main():
    args, match = [], []
    it = iter(sys.argv[1:])
    for a in it:
        if a == "--match":
            match.append(next(it))
        else:
            args.append(a)
    tables = [parse(p) for p in args]
    names = sorted({n for t in tables for n in t})
    pretty = demangle(names)
    names = [n for n in names if not match or any(s in pretty[n] for s in match)]
    cols = [s for _, s in FIELDS]
    print("kernel | " + " | ".join(" ".join(cols) for _ in tables))
    differ = 0
    for n in sorted(names, key=lambda n: [int(x) if x.isdigit() else x for x in re.split(r"(\d+)", pretty[n])]):
        rows = [t.get(n) for t in tables]
        cells = [" ".join(str(r[c]) for c in cols) if r else "-" for r in rows]
        mark = ""
        if len(rows) == 2 and rows[0] != rows[1]:
            mark, differ = "  !=", differ + 1
        print(f"{pretty[n]} | " + " | ".join(cells) + mark)
    if len(tables) == 2:
        print(f"{len(names)} kernels, {differ} differ")


if __name__ == "__main__":
    main()

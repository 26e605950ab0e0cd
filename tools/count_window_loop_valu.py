"""Static VALU count of a kernel's window loop, from the assembly of a device-only -S compile:
python3 tools/count_window_loop_valu.py FILE.s 'gdn_dense_fused_kernelILi4ELi2ELi1ELi16ELi0E' [--phases]

The window loop is the largest loop of the kernel (label .. backward branch to it) that holds an MFMA.  Counted are
the v_* instructions per wave and trip, the MFMA among them, the v_pk_* among them and the s_nop.  --phases also
cuts the loop at its s_setprio / s_barrier marks (the fused kernel: X | S | M | P1 | E, see gdn_forward_dense.hip)."""
import re
import sys


def kernel_body(lines, pat):
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\w*" + re.escape(pat) + r"\w*:", l))
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith("s_endpgm"))
    return lines[start:end + 1]


def window_loop(body):
    labels = {m.group(1): i for i, l in enumerate(body) if (m := re.match(r"^(\.LBB\d+_\d+):", l))}
    best = None
    for i, l in enumerate(body):
        m = re.match(r"\s+s_cbranch_\w+\s+(\.LBB\d+_\d+)", l) or re.match(r"\s+s_branch\s+(\.LBB\d+_\d+)", l)
        if m and labels.get(m.group(1), 1 << 30) < i:
            seg = body[labels[m.group(1)]:i + 1]
            if any("v_mfma" in s for s in seg) and (best is None or len(seg) > len(best)):
                best = seg
    return best


def ops(seg):
    return [l.split()[0] for l in seg if re.match(r"^\s+[a-z]", l) and not l.strip().startswith(";")]


def count(seg):
    o = ops(seg)
    v = [x for x in o if x.startswith("v_")]
    return dict(valu=len(v), mfma=sum(x.startswith("v_mfma") for x in v), pk=sum(x.startswith("v_pk_") for x in v),
                mov=sum(x.startswith("v_mov") for x in v), s_nop=sum(x == "s_nop" for x in o),
                ds=sum(x.startswith("ds_") for x in o))


def main():
    lines = open(sys.argv[1]).read().splitlines()
    body = kernel_body(lines, sys.argv[2])
    loop = window_loop(body)
    print(sys.argv[2], "window loop:", count(loop))
    if "--phases" in sys.argv:
        cut = [0]
        marks = []
        for i, l in enumerate(loop):
            t = l.split()
            if t and t[0] in ("s_setprio", "s_barrier"):
                cut.append(i)
                marks.append(" ".join(t[:2]))
        cut.append(len(loop))
        print("  marks:", marks)
        names = ["(head)"] + marks
        for n, a, b in zip(names, cut[:-1], cut[1:]):
            c = count(loop[a:b])
            hist = {}
            for x in ops(loop[a:b]):
                if x.startswith("v_"):
                    hist[x] = hist.get(x, 0) + 1
            print(f"  from {n:14s}: {c}")
            if "--hist" in sys.argv:
                print("     ", dict(sorted(hist.items(), key=lambda kv: -kv[1])))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""One line per kernel of the given HIP sources: resource figures and a hash of the kernel's gfx950 instruction text.

    tools/kernel_isa_digest.py gemm_fwd.hip gemm_cell.hip ... > new.txt
    tools/kernel_isa_digest.py /path/to/another/checkout/regt-gcn_amd/csrc/gemm.hip > old.txt ; diff old.txt new.txt

Like kernel_regs.py it compiles each source to assembly (hipcc -S --cuda-device-only) with build.py's FLAGS.  A name without a
directory is looked up in regt-gcn_amd/csrc.  Lines are sorted by demangled kernel name, so the listings of two cuts of the same
kernels into translation units compare with `diff`: a refactor that is invisible to the compiler gives identical listings.
Before hashing, comments are dropped and the labels that carry a per-unit number (.LBB<n>_<m>, .Lfunc_end<n>, .Ltmp<n>, ...) are
renumbered in order of appearance.  Whole texts are compared; nothing in them is searched for.  (A kernel's text is taken from its
label to the next `.section` directive: that is how this compiler lays its output out.)
"""
import hashlib, importlib.util, os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "regt-gcn_amd", "csrc")
_spec = importlib.util.spec_from_file_location("_regt_build", os.path.join(ROOT, "regt-gcn_amd", "build.py"))
_build = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_build)
FIELDS = [("vgpr", "vgpr_count"), ("agpr", "agpr_count"), ("sgpr", "sgpr_count"), ("scratch", "private_segment_fixed_size"),
          ("lds", "group_segment_fixed_size")]
LABEL = re.compile(r"\.L[A-Za-z_]+\d+(?:_\d+)?")


def kernel_text(asm, name):
    """The instructions of one kernel: from its label to the section switch that ends its code."""
    start = asm.index("\n" + name + ":") + 1
    body = asm[start:asm.index("\n\t.section", start)].split("\n")[1:]
    lines = [l.split(";")[0].rstrip() for l in body]
    seen = {}
    renumber = lambda m: seen.setdefault(m.group(0), ".L%d" % len(seen))
    return "\n".join(LABEL.sub(renumber, l) for l in lines if l.strip())


def digest(asm):
    rows = []
    for block in asm.split("  - .agpr_count:")[1:]:
        block = ".agpr_count:" + block
        get = lambda k: re.search(r"\." + k + r":\s+(\S+)", block).group(1)
        name = get("name")
        rows.append((name, [get(k) for _, k in FIELDS], hashlib.sha256(kernel_text(asm, name).encode()).hexdigest()[:16]))
    return rows


def main(argv):
    srcs = [a if os.path.dirname(a) else os.path.join(CSRC, a) for a in argv]
    if not srcs:
        raise SystemExit(__doc__)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        # (a .s argument is an assembly made earlier with the same command: taken as it is)
        outs = [s if s.endswith(".s") else os.path.join(tmp, "%d.s" % i) for i, s in enumerate(srcs)]
        procs = [subprocess.Popen([hipcc] + _build.FLAGS + ["-S", "--cuda-device-only", "-o", o, s], stderr=subprocess.PIPE, text=True)
                 for s, o in zip(srcs, outs) if s != o]
        for p in procs:
            err = p.communicate()[1]
            if p.returncode != 0:
                raise SystemExit("hipcc failed on %s\n%s" % (p.args[-1], err))
        for o in outs:
            with open(o) as f:
                rows += digest(f.read())
    names = subprocess.run(["c++filt"], input="\n".join(r[0] for r in rows), capture_output=True, text=True).stdout.split("\n")
    for (_, figs, h), name in sorted(zip(rows, names), key=lambda t: t[1]):
        print(" ".join("%s %s" % (label, v) for (label, _), v in zip(FIELDS, figs)) + "  isa %s  %s" % (h, name))


if __name__ == "__main__":
    main(sys.argv[1:])

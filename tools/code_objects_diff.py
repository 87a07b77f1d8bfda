"""Every gfx950 kernel of two builds of libipmc.so against each other, per translation unit: symbol sets,
instruction lists, register and spill counts, scratch and LDS (tools/code_objects.py, llvm-objdump -d; no GPU).

  python tools/code_objects_diff.py parent/libipmc.so new/libipmc.so [--full] [name substring ...]

Kernels whose demangled name holds one of the substrings are listed with their budget either way; --full
prints both instruction lists of every kernel that differs."""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import code_objects as CO  # noqa: E402

KEYS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count",
        ".private_segment_fixed_size", ".group_segment_fixed_size")


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    return dict(zip(names, out.split("\n")))


def listing(co):
    """{symbol: [instruction text]} of one code object"""
    out = subprocess.run([os.path.join(CO.LLVM, "llvm-objdump"), "-d", "--mcpu=gfx950", co], check=True,
                         capture_output=True, text=True).stdout
    syms, cur = {}, None
    for line in out.split("\n"):
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = syms.setdefault(m.group(1), [])
            continue
        m = re.match(r"\t(\S.*?)\s*// ([0-9A-F]+):", line)
        if m and cur is not None:
            cur.append(" ".join(m.group(1).split()))
    return syms


def unit(co):
    return {k[".name"]: k for k in CO._metadata(co)["amdhsa.kernels"]}, listing(co)


def main():
    args = [a for a in sys.argv[1:] if a != "--full"]
    parent, new, named = args[0], args[1], args[2:]
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        ca, cb = CO._code_objects(parent, ta), CO._code_objects(new, tb)
        print(f"code objects: parent {len(ca)}, new {len(cb)}")
        total = same = 0
        differing, listed = [], []
        for n, (a, b) in enumerate(zip(ca, cb)):
            (ma, la), (mb, lb) = unit(a), unit(b)
            names = demangle(sorted(set(ma) | set(mb)))
            ident = 0
            for k in sorted(set(ma) & set(mb)):
                total += 1
                differs = la[k] != lb[k] or any(ma[k].get(x, 0) != mb[k].get(x, 0) for x in KEYS)
                ident += not differs
                same += not differs
                if differs:
                    differing.append((names[k], ma[k], mb[k], la[k], lb[k]))
                if any(s in names[k] for s in named):
                    listed.append((names[k], mb[k], differs))
            first = names[sorted(ma)[0]] if ma else "-"
            print(f"unit {n:2d} ({first[:60]}...): {len(ma)} kernels, symbol sets "
                  f"{'identical' if set(ma) == set(mb) else 'DIFFER'}, {ident} identical in instructions, "
                  "registers, scratch and LDS")
            for k in sorted(set(ma) ^ set(mb)):
                print(f"   only in {'parent' if k in ma else 'new'}: {names[k]}")
        print(f"\n{same} of {total} kernels identical; {len(differing)} differ")
        for name, a, b, ia, ib in differing:
            print(f"\n== {name}")
            for x in KEYS:
                print(f"   {x}: parent {a.get(x, 0)} new {b.get(x, 0)}")
            print(f"   instructions: parent {len(ia)} new {len(ib)}")
            if "--full" in sys.argv:
                print("   --- parent\n" + "\n".join("   " + x for x in ia))
                print("   --- new\n" + "\n".join("   " + x for x in ib))
        if listed:
            print("\nthe kernels asked for by name:")
        for name, m, differs in listed:
            print(f"   {name}: {'differs' if differs else 'identical to the parent'}; vgpr {m['.vgpr_count']} sgpr "
                  f"{m['.sgpr_count']} scratch {m['.private_segment_fixed_size']} B vgpr_spill "
                  f"{m.get('.vgpr_spill_count', 0)} sgpr_spill {m.get('.sgpr_spill_count', 0)} lds "
                  f"{m['.group_segment_fixed_size']} B")


if __name__ == "__main__":
    main()

"""Developer helper: is every kernel of tree B the machine code it is in tree A?  Compiles every csrc/*.hip of both trees with
the library's flags (-S --cuda-device-only) and compares kernel by kernel: the instruction count and a hash of the body (label
to the last s_endpgm, comments stripped, local labels normalised) and the descriptor fields.  A kernel may change files.
    python tools/isa_kernel_diff.py <tree A> <tree B>"""
import collections, hashlib, importlib.util, os, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor
FIELDS = ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size", "kernarg_size",
          "float_denorm_mode_32")


def kernels(tree):
    """mangled name -> (file, instruction histogram, body hash, descriptor fields)"""
    spec = importlib.util.spec_from_file_location("reloc_build_flags", os.path.join(tree, "nclt-slam-project_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    tmp = tempfile.mkdtemp()

    def listing(s):
        asm = os.path.join(tmp, s[:-4] + ".s")
        subprocess.run([b.HIPCC] + b.FLAGS + ["-S", "--cuda-device-only", "-o", asm, os.path.join(b.CSRC, s)], check=True,
                       stderr=subprocess.DEVNULL)
        return s, open(asm).read()

    out = {}
    with ThreadPoolExecutor(max_workers=4) as ex:
        for s, text in ex.map(listing, b.sources()):
            lines = text.splitlines()
            for name, desc in re.findall(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)^\s*\.end_amdhsa_kernel", text, flags=re.M | re.S):
                start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
                end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
                body = [re.sub(r"\.LBB\d+_", ".L", l.split(";")[0]).strip() for l in lines[start + 1:end]]
                body = [l for l in body if l and (l.endswith(":") or not l.startswith("."))]
                body = body[:max(i for i, l in enumerate(body) if l.startswith("s_endpgm")) + 1]
                hist = collections.Counter(l.split()[0] for l in body if not l.endswith(":"))
                fields = tuple(re.search(r"\.amdhsa_%s\s+(\S+)" % f, desc).group(1) for f in FIELDS)
                out[name] = (s, hist, hashlib.sha1("\n".join(body).encode()).hexdigest()[:12], fields)
    return out


if __name__ == "__main__":
    A, B = kernels(sys.argv[1]), kernels(sys.argv[2])
    print("# verdict kernel [file A -> file B]: instructions, body hash; " + " ".join(FIELDS))
    verdicts = collections.Counter()
    for name in sorted(set(A) | set(B)):
        if name not in A or name not in B:
            verdict, rows = ("ONLY-A", [A[name]]) if name in A else ("ONLY-B", [B[name]])
        else:
            verdict, rows = ("SAME", [B[name]]) if A[name][1:] == B[name][1:] else ("DIFF", [A[name], B[name]])
        verdicts[verdict] += 1
        files = A.get(name, B.get(name))[0] + ("" if verdict != "SAME" or A[name][0] == B[name][0] else " -> " + B[name][0])
        print(f"{verdict:6s} {name} [{files}]")
        for f, hist, digest, fields in rows:
            print(f"       {sum(hist.values())} instructions, {digest}; " + " ".join(fields))
        if verdict == "DIFF":
            delta = {k: B[name][1][k] - A[name][1][k] for k in set(A[name][1]) | set(B[name][1]) if A[name][1][k] != B[name][1][k]}
            print(f"       histogram B - A: {delta or 'equal'}")
    print("# " + ", ".join(f"{n} {v}" for v, n in sorted(verdicts.items())), f"of {len(set(A) | set(B))} kernels")

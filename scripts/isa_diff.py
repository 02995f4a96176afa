#!/usr/bin/env python3
"""Dev helper: did a source change leave the machine code alone?  Compiles every .hip file of <git-ref> and of the working
tree to gfx950 assembly (scripts/check_isa.py's flags) and compares the text kernel by kernel -- the code from the kernel's
label to its end plus its .amdhsa_kernel descriptor, without comment lines, trailing comments, the .file / .ident / .loc
directives and the function number in local labels.  One line per kernel; exit code 1 if a render_kernel instantiation
differs or a file's set of kernel symbols changed.
    python scripts/isa_diff.py <git-ref>"""
import glob, io, os, re, subprocess, sys, tarfile, tempfile
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from check_isa import DEFAULT_FLAGS
CSRC = os.path.join("myraytracer_amd", "csrc")


def kernels_of(path, td):
    """{kernel symbol: (normalised text, instruction count)} of one .hip file"""
    out = os.path.join(td, re.sub(r"\W", "_", path) + ".s")
    subprocess.check_call(["/opt/rocm/bin/hipcc", *DEFAULT_FLAGS.split(), "--cuda-device-only", "-S", "-o", out, path],
                          stderr=subprocess.DEVNULL)
    lines = []
    for l in open(out):
        l = re.sub(r"\.L(BB|func_end|func_begin)\d+", r".L\1", l.split(";")[0].rstrip())
        if l.strip() and not re.match(r"\s*\.(file|ident|loc)\b", l):
            lines.append(l)
    res, k = {}, 0
    while k < len(lines):
        m = re.match(r"\s*\.amdhsa_kernel (\S+)", lines[k])
        if m:
            sym = m.group(1)
            end = next(j for j in range(k, len(lines)) if ".end_amdhsa_kernel" in lines[j])
            first = lines.index(sym + ":")
            last = next(j for j in range(first, len(lines)) if lines[j].startswith(".Lfunc_end"))
            body = lines[first:last]
            n_instr = sum(1 for l in body if not l.endswith(":") and not l.lstrip().startswith("."))
            res[sym] = ("\n".join(body + lines[k:end]), n_instr)
            k = end
        k += 1
    return res


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = sys.argv[1]
    with tempfile.TemporaryDirectory() as td:
        # the ref's sources with their directory layout (mrt_internal.h includes ../../include/...)
        tar = subprocess.check_output(["git", "-C", ROOT, "archive", ref, CSRC, "include"])
        tarfile.open(fileobj=io.BytesIO(tar)).extractall(os.path.join(td, "ref"))
        names = sorted({os.path.basename(f) for root in (ROOT, os.path.join(td, "ref"))
                        for f in glob.glob(os.path.join(root, CSRC, "*.hip"))})
        jobs = [(root, n) for n in names for root in (os.path.join(td, "ref"), ROOT) if os.path.exists(os.path.join(root, CSRC, n))]
        with ThreadPoolExecutor(max_workers=min(len(jobs), os.cpu_count() or 1, 16)) as pool:
            done = dict(zip(jobs, pool.map(lambda j: kernels_of(os.path.join(j[0], CSRC, j[1]), td), jobs)))
    bad = same = differ = 0
    for n in names:
        old, new = done.get((os.path.join(td, "ref"), n), {}), done.get((ROOT, n), {})
        for sym in sorted(set(old) | set(new)):
            dem = subprocess.run(["c++filt", sym], capture_output=True, text=True).stdout.strip().replace("(anonymous namespace)::", "")
            if sym not in old or sym not in new:
                print(f"{n}: {'ADDED  ' if sym in new else 'REMOVED'}    {dem}")
                bad += 1
                continue
            ident = old[sym][0] == new[sym][0]
            same, differ = same + ident, differ + (not ident)
            bad += (not ident) and "render_kernel" in sym
            print(f"{n}: {'identical' if ident else 'DIFFERENT'}  {old[sym][1]:5d} -> {new[sym][1]:5d} instructions  {dem}")
    print(f"isa_diff against {ref}: {same} kernel(s) identical, {differ} different; "
          f"{bad} problem(s) (render_kernel differences, symbols added or removed)")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

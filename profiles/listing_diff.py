"""Are the gfx950 instruction streams of the kernels the same as at a git revision?  (labels and symbol names aside)
Usage: python3 profiles/listing_diff.py [rev]   -- builds `make asm` of that revision in a temporary directory.
Used when a change is meant to leave existing kernels untouched (e.g. a new template parameter).  The listings compared
are those of the Makefile's KERNELS; a kernel that differs is printed with whether its .amdhsa_ descriptor, its
instruction count and its multiset of opcodes are still the revision's."""
import collections, os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
rev = sys.argv[1] if len(sys.argv) > 1 else "HEAD"

def bodies(path):
    out = {}
    for m in re.finditer(r"^(_ZN\w+):[^\n]*\n(.*?)\n\.Lfunc_end", open(path).read(), re.S | re.M):
        out[m.group(1)] = [re.sub(r"\.L\w+|_ZN\w+", "X", l.strip()) for l in m.group(2).splitlines()
                           if l.strip() and not l.strip().startswith((";", "."))]
    return out

def descriptors(path):
    return dict(re.findall(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", open(path).read(), re.S | re.M))

def listings():   # NAME.s for every NAME of the Makefile's KERNELS
    mk = open(f"{ROOT}/dbde-video-cpp_amd/csrc/Makefile").read().replace("\\\n", " ")
    return [n + ".s" for n in re.search(r"^KERNELS\s*:=.*?addsuffix \.hip,([^)]*)\)", mk, re.M).group(1).split()]

with tempfile.TemporaryDirectory() as tmp:
    subprocess.run(f"git -C {ROOT} archive {rev} dbde-video-cpp_amd/csrc include | tar -x -C {tmp}", shell=True, check=True)
    subprocess.run(["make", "-s", "-C", f"{tmp}/dbde-video-cpp_amd/csrc", "asm"], check=True, capture_output=True)
    subprocess.run(["make", "-s", "-C", f"{ROOT}/dbde-video-cpp_amd/csrc", "asm"], check=True, capture_output=True)
    bad = 0

    def renamed(k):   # an old instance's name today: the 8- and 16-bit window and projection kernels are templates on the pixel size
        k = re.sub(r"19decode_roi16_kernelILj(\d+)EEEvNS_9RoiParamsE", r"17decode_roi_kernelILj\1ELj2EEEvNS_9RoiParamsE", k)
        k = re.sub(r"17decode_roi_kernelILj(\d+)EEEvNS_9RoiParamsE", r"17decode_roi_kernelILj\1ELj1EEEvNS_9RoiParamsE", k)
        k = re.sub(r"16project16_kernelILj(\d+)EEEvNS_10ProjParamsE", r"14project_kernelILj\1ELj2EEEvNS_10ProjParamsE", k)
        k = re.sub(r"14project_kernelILj(\d+)EEEvNS_10ProjParamsE", r"14project_kernelILj\1ELj1EEEvNS_10ProjParamsE", k)
        k = k.replace("24project16_combine_kernelENS_10ProjParamsE", "22project_combine_kernelILj2EEEvNS_10ProjParamsE")
        return k.replace("22project_combine_kernelENS_10ProjParamsE", "22project_combine_kernelILj1EEEvNS_10ProjParamsE")

    for f in listings():
        if not os.path.exists(f"{tmp}/dbde-video-cpp_amd/csrc/{f}"):
            print("new file", f)
            continue
        d_old, d_new = descriptors(f"{tmp}/dbde-video-cpp_amd/csrc/{f}"), descriptors(f"{ROOT}/dbde-video-cpp_amd/csrc/{f}")
        old, new = bodies(f"{tmp}/dbde-video-cpp_amd/csrc/{f}"), bodies(f"{ROOT}/dbde-video-cpp_amd/csrc/{f}")
        seen = set()
        for k, v in old.items():
            cands = [k, renamed(k), k.replace("EEEvNS_9EncParamsE", "ELi1EEEvNS_9EncParamsE"), k.replace("EEEvNS_9DecParamsE", "ELi256EEEvNS_9DecParamsE")]
            k2 = next((c for c in cands if c in new), None)
            if k2 is None:
                print("gone ", k); bad += 1
                continue
            seen.add(k2)
            if new[k2] != v:
                ops = lambda b: collections.Counter(l.split()[0] for l in b)
                print("DIFF ", k2, len(v), "->", len(new[k2]),
                      "descriptor", "missing" if k not in d_old or k2 not in d_new else
                      "equal" if d_old[k] == d_new[k2] else "DIFFERS",
                      "opcodes", "equal" if ops(v) == ops(new[k2]) else "DIFFER"); bad += 1
        for k in new:
            if k not in seen:
                print("new  ", k, len(new[k]))
    print("identical" if not bad else f"{bad} kernels differ")
